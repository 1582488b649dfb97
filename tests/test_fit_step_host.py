"""One trust-region step of the device fit, on the host: the restatement the GPU test is held to, against scipy's own functions.

tests/test_gpu_fit_step.py compares the step probe (sr_expfit_step_probe_f64: the solver's own Coleman-Li scaling, solve_tr,
select_step, strictly_feasible) with oracle/sr_oracle.py:trf_step_exact, a long-double restatement of sr_fit.hip.  This file
pins that restatement, without a GPU, on every case of tests/golden/fit_step_cases.npz (oracle/gen_golden_fit_step.py):

  * against scipy 1.15.3 (the version sr_fit.hip cites): CL_scaling_vector, solve_lsq_trust_region (rank decision, alpha,
    iteration count, p_h), trf.select_step (branch, step, step_h, predicted), step_size_to_bound (value and hits),
    make_strictly_feasible (rstep 1e-10 and 0), minimize_quadratic_1d, intersect_trust_region.  scipy's solver wants the SVD of the
    augmented scaled Jacobian; any factor of B = J_h^T J_h + diag_h has the same singular values and right vectors, so it gets
    s = sqrt(lambda), V from a 60-digit symmetric eigendecomposition (mpmath) of the long-double B, and uf = V^T g_h / s, each
    rounded to float64.  scipy then works in float64 on (s, V, uf) that carry n roundings of size u: a perturbation of B + alpha I
    of at most ~n u |B| in norm, which moves the step -(B + alpha I)^-1 g_h by at most kappa_2(B + alpha I) n u relative; the
    restatement itself is exact to ~1e-19.  Asserted: 16 n kappa_2(B + alpha I) u times the scale of the quantity
    (sr_oracle.step_scales); the worst case met is printed.
  * the coverage the generator searched for: every select_step branch and both solve_tr outcomes of branch 0 at least 6 times per
    order P >= 5 and 3 times for P = 2, 3, 4; the rarer paths (EVENTS) at least once;
  * decisiveness: outside the `breakdown` class every decision margin of trf_step_exact is >= 1e-6 and the float64 restatement
    (trf_step_f64) takes the same decisions, so no case has to be skipped on the GPU;
  * the constant c of the GPU test's conditioning bar: 4 x the worst distance of trf_step_f64 from trf_step_exact over the decisive
    cases in units of kappa_2(B + alpha I) u scale, equal to the fixture's c_bar;
  * teeth: each of five deliberate errors injected into trf_step_f64 moves an output beyond that bar (or flips a flag the GPU
    test compares exactly) on at least one committed case -- see INJECTIONS.

Not reachable with decisive margins, hence not among the cases: r_stride <= 0 in select_step.  It needs a component that lies on its
bound after the step to the first bound without being in `hits`, i.e. two strides that differ in the last bit.  r_value = inf is
covered through its other door, r_stride_l > r_stride_u.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
import sr_oracle as o                                                                     # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -53
MARGIN = 1e-6
EVENTS = ('alpha_clamped', 'iterations_exhausted', 'hits_tie', 'zero_step_component', 'r_value_inf', 'cauchy_to_bound')
# deliberate error -> the outputs of the GPU test that must move (flags compared exactly, or floats beyond the conditioning bar)
INJECTIONS = {
    'reflect_wrong_sign': 'the reflected direction flips the components that did NOT hit a bound',
    'theta_on_to_tr': 'theta multiplies to_tr instead of to_bound in r_stride_u',
    'other_root': 'the smaller root of the trust-region intersection is taken',
    'rank_m_is_N': 'the rank threshold uses m = N instead of the number of points',
    'alpha_not_rescaled': 'alpha *= Delta / Delta_new is dropped between two steps (warm-start cases: alpha_in = the old alpha)',
}


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLD, 'fit_step_cases.npz'))


@pytest.fixture(scope='module')
def results(fixture):
    """[(case, class, exact, float64)] once for the module"""
    return [(case, cls, o.trf_step_exact(*case), o.trf_step_f64(*case)) for case, cls in o.step_cases(fixture)]


def f64(a):
    return np.asarray(a, dtype=np.float64)


def bucket(r):
    return ('b0_alpha0' if r['alpha'] == 0 else 'b0_alpha') if r['branch'] == 0 else 'b%d' % r['branch']


def decisive(cls, ex, f):
    marg = {k: v for k, v in ex['margins'].items() if not (cls == 'rank_edge' and k in ('rank', 'pivot'))}
    same = all(ex[k] == f[k] for k in ('branch', 'full_rank', 'iterations', 'pivot_failures', 'events')) and \
        np.array_equal(f64(ex['dv']), f64(f['dv'])) and np.array_equal(np.sign(f64(ex['step_h'])), np.sign(f64(f['step_h'])))
    return min(marg.values()), same


def test_fixture_is_small_data(fixture):
    n = sum(fixture['par_%d' % P].shape[0] for P in fixture['orders'])
    assert n <= 400
    assert [int(P) for P in fixture['orders']] == [2, 3, 4, 5, 7, 9, 11]
    assert os.path.getsize(os.path.join(GOLD, 'fit_step_cases.npz')) < 600 * 1024
    for k in fixture.files:
        assert fixture[k].dtype.kind in 'fiU', k        # numbers and the class names: no objects, nothing to execute


def test_coverage(results):
    count, events, breakdown = {}, set(), 0
    for case, cls, ex, f in results:
        if cls == 'breakdown':
            breakdown += 1
            assert f['pivot_failures'] > 0
            continue
        P = case[0].size
        count[(P, bucket(ex))] = count.get((P, bucket(ex)), 0) + 1
        events.update(ex['events'])
    for P in (2, 3, 4, 5, 7, 9, 11):
        for b in ('b0_alpha0', 'b0_alpha', 'b1', 'b2', 'b3'):
            assert count.get((P, b), 0) >= (6 if P >= 5 else 3), (P, b, count.get((P, b), 0))
    assert breakdown >= 8
    assert not set(EVENTS) - events, set(EVENTS) - events
    dv0 = [1 for case, cls, ex, f in results if cls == 'edge' and (f64(ex['dv']) == 0).any()]
    th = [float(ex['theta']) for case, cls, ex, f in results if cls == 'edge']
    assert dv0 and 0.995 in th and any(t > 0.995 for t in th)
    re = [ex['full_rank'] for case, cls, ex, f in results if cls == 'rank_edge']
    assert 0 in re and 1 in re
    warm = sum(1 for case, cls, ex, f in results if case[6] > 0 and cls != 'breakdown')
    assert warm >= 10, warm


def test_every_case_outside_breakdown_is_decisive(results):
    for i, (case, cls, ex, f) in enumerate(results):
        if cls == 'breakdown':
            continue
        m, same = decisive(cls, ex, f)
        assert m >= MARGIN and same and ex['pivot_failures'] == 0, (i, cls, ex['margins'])


def branch_of(step_h, p_h_bound, g_h):
    """which candidate of select_step a scaled step is: theta times the step to the bound (1), a multiple of -g_h (3), or neither (2)"""
    if np.allclose(step_h, p_h_bound, rtol=1e-12, atol=0):
        return 1
    return 3 if -(step_h @ g_h) >= (1 - 1e-12) * np.linalg.norm(step_h) * np.linalg.norm(g_h) else 2


def test_restatement_against_scipy(results):
    from scipy.optimize._lsq import common as C, trf
    worst = 0.0
    for i, (case, cls, ex, f) in enumerate(results):
        x, A, g, tau_max, m, Delta, alpha_in = case
        n = x.size
        lb, ub = o.fit_bounds(n, tau_max)
        # Coleman-Li scaling and the strictly feasible points: float64 operations on float64 inputs, bit for bit
        v, dv = C.CL_scaling_vector(x, g, lb, ub)
        assert np.array_equal(v, f64(f['v'])) and np.array_equal(dv, f64(f['dv'])) and np.array_equal(dv, f64(ex['dv'])), i
        assert np.all(np.abs(v - f64(ex['v'])) <= U * np.abs(v)), i
        for pt in (x, f64(f['xn_raw']), np.where(np.arange(n) % 2 == 0, lb, ub), np.where(np.arange(n) % 3 == 0, ub, x)):
            for rstep in (1e-10, 0.0):
                mine = f64(o._strictly_feasible(np.float64, list(pt), list(lb), list(ub), rstep))
                assert np.array_equal(C.make_strictly_feasible(pt.copy(), lb, ub, rstep=rstep), mine), (i, rstep)
        if cls == 'breakdown':
            continue
        B, g_h, d, p_h = f64(ex['B']), f64(ex['g_h']), f64(ex['d']), f64(ex['p_h'])
        kap = o.step_kappa(B, ex['alpha'])
        bar = 16 * n * kap * U
        sc = o.step_scales(ex)
        # solve_lsq_trust_region
        s, V, uf = o.step_svd(ex['B'], ex['g_h'])
        full = bool(s[-1] > o.STEP_EPS * m * s[0])
        assert full == bool(ex['full_rank']), (i, cls, s[-1] / s[0])
        p_sc, alpha_sc, nit = C.solve_lsq_trust_region(n, m, uf, s, V, Delta, initial_alpha=alpha_in)
        assert nit == ex['iterations'], (i, nit, ex['iterations'])
        assert abs(alpha_sc - float(ex['alpha'])) <= bar * sc['alpha'], (i, alpha_sc, float(ex['alpha']), kap)
        assert np.max(np.abs(p_sc - p_h)) <= bar * sc['p_h'], (i, np.max(np.abs(p_sc - p_h)) / Delta, kap)
        worst = max(worst, np.max(np.abs(p_sc - p_h)) / (kap * U * Delta))
        # select_step, from the restatement's own p_h: J_h = diag(s) V^T is a factor of B, diag_h is inside it
        J_h = s[:, None] * V.T
        theta = float(f64(ex['theta']))
        step, step_h, pred = trf.select_step(x, J_h, np.zeros(n), g_h, d * p_h, p_h.copy(), d, Delta, lb, ub, theta)   # (works in place)
        kb = 16 * n * o.step_kappa(B, 0.0) * U
        if ex['branch'] == 0:
            assert np.array_equal(step, d * p_h) and np.array_equal(step_h, p_h), i
        else:
            p_stride, _ = C.step_size_to_bound(x, d * p_h, lb, ub)
            assert branch_of(step_h, theta * (p_stride * p_h), g_h) == ex['branch'], (i, ex['branch'])
            assert np.max(np.abs(step_h - f64(ex['step_h']))) <= kb * sc['step_h'], (i, ex['branch'])
            assert np.max(np.abs(step - f64(ex['step']))) <= kb * sc['step'], (i, ex['branch'])
        quad = np.linalg.norm(B, 2) * float(ex['step_h_norm']) ** 2 + np.linalg.norm(g_h) * float(ex['step_h_norm'])
        assert abs(pred - float(ex['predicted'])) <= kb * sc['predicted'] + 16 * n * U * quad, (i, pred, float(ex['predicted']))
        # the small pieces, float64 against float64: the same IEEE operations
        marg = o._Margins()
        p = d * p_h
        st, hits = C.step_size_to_bound(x, p, lb, ub)
        st2, hits2 = o._step_to_bound(np.float64, list(x), list(p), list(lb), list(ub), marg)
        assert st == st2 and list(hits) == hits2, i
        qa, qb = 0.5 * p_h @ B @ p_h, g_h @ p_h
        for lo, hi, c in ((0.0, 1.0, 0.0), (0.25, 0.75, 1.5), (0.0, float(-0.5 * qb / qa) * 0.5, -1.0)):
            t1, y1 = C.minimize_quadratic_1d(qa, qb, lo, hi, c=c)
            t2, y2 = o._min_quad_1d(np.float64, np.float64(qa), np.float64(qb), np.float64(lo), np.float64(hi), np.float64(c), marg)
            assert t1 == t2 and y1 == y2, (i, lo, hi)
        # intersect_trust_region from a point well inside (no cancellation in c): numpy's dot against the sequential sums
        xh, sh = 0.5 * p_h, np.where(np.arange(n) % 2 == 0, -p_h, p_h)
        ta = sorted(f64(o._intersect_tr(np.float64, list(xh), list(sh), np.float64(Delta))))
        tb = C.intersect_trust_region(xh, sh, Delta)
        assert np.allclose(ta, tb, rtol=64 * n * U, atol=0), i
    print('worst |p_h(scipy) - p_h| / (kappa u Delta) = %.3g (bar %d n)' % (worst, 16))


def test_conditioning_constant(results, fixture):
    worst, where = 0.0, None
    for i, (case, cls, ex, f) in enumerate(results):
        if cls == 'breakdown':
            continue
        r = o.step_ratios(ex, f)
        k = max(r, key=r.get)
        if r[k] > worst:
            worst, where = r[k], (i, case[0].size, k)
    print('float64 restatement against long double: worst ratio %.4g at (case, P, output) %r; c = %.4g' % (worst, where, 4 * worst))
    assert np.isfinite(worst)
    assert float(fixture['c_bar']) == pytest.approx(4 * worst, rel=1e-12)


def moved(ex, other, c):
    """what the GPU test would see: a flag that differs, or an output beyond the bar"""
    if any(ex[k] != other[k] for k in ('branch', 'full_rank', 'pivot_failures')):
        return 'flags'
    r = o.step_ratios(ex, other)
    k = max(r, key=r.get)
    return k if r[k] > c else None


def test_injected_errors_are_seen(results, fixture):
    c = float(fixture['c_bar'])
    warm = {}
    k = 0
    for P in [int(n) for n in fixture['orders']]:
        for w in fixture['warm_%d' % P]:
            warm[k] = w
            k += 1
    for inj in INJECTIONS:
        hit = []
        for i, (case, cls, ex, f) in enumerate(results):
            if cls == 'breakdown':
                continue
            if inj == 'alpha_not_rescaled':
                if warm[i][0] == 0:
                    continue
                bad = o.trf_step_f64(*case[:6], float(warm[i][0]))
            else:
                bad = o.trf_step_f64(*case, inject=inj)
            what = moved(ex, bad, c)
            if what:
                hit.append((i, what))
        print('%s: seen on %d cases, first %r' % (inj, len(hit), hit[:6]))
        assert len(hit) >= 2, inj
