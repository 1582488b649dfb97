"""
GPU test of ONE trust-region step of the fit solver (kernel 3b, sr_fit.hip), the layer between a Jacobian and the trial evaluation:
Coleman-Li scaling, B = D A D + diag(g dv), solve_tr (More's iteration on Cholesky factors), select_step (Gauss-Newton step, step to
the bound, reflected step, Cauchy step), step_to_bound, min_quad_1d, strictly_feasible.  Converged fits cannot see this layer: a
wrong step is rejected by the ratio test and costs evaluations, not chi^2.  sr_expfit_step_probe_f64 runs the solver's own
solve_tr / select_step / strictly_feasible templates on given (x, J^T J, J^T f, Delta, alpha) and every output is compared with
oracle/sr_oracle.py:trf_step_exact, the same operations in long double, which tests/test_fit_step_host.py pins against scipy's own
functions.  Cases: tests/golden/fit_step_cases.npz (oracle/gen_golden_fit_step.py); the cases of one order that share tau_max (a
kernel argument) go in one launch, a handful of launches per order.

No case is skipped.  Every case outside the `breakdown` class is decisive (each decision margin of the long-double step >= 1e-6,
asserted by the host test), so flags are compared exactly and floats against bars (u = 2^-53):

  exact      dv, the branch of select_step, the full-rank flag of solve_tr, the iteration count, the signs of step_h (where `hits`
             shows), 0 pivot failures; x after strictly_feasible(., 1e-10) bit for bit against the float64 restatement (IEEE
             additions and multiplications of float64 inputs: nextafter, lb + rstep max(1, |lb|), the mid-point rule)
  v          ub - x or x - lb, one rounding: u |v|
  d          sqrt of that, correctly rounded: (1/2 + 1/2) u, asserted 2 u |d|
  g_h        d g: 3 u |g_h|
  B          (A d_i) d_j + [i = j] g dv: two factors at 2 u, two products, one sum of terms of one sign: 7 u |B_ij|
  g_norm     max |g v|: 2 u;   theta = max(0.995, 1 - g_norm): 2 u g_norm + u
  init       v: u |v|;  Delta = sqrt(sum (x / sqrt(v))^2): each quotient 3 u, its square 7 u, n positive terms n u, the root
             halves it and rounds once: asserted (n + 9) u Delta
  alpha, p_h, step, step_h, predicted, xn
             c kappa_2(B + alpha I) u times the scale of the quantity (sr_oracle.step_scales: Delta; Delta max d for step and
             xn, plus 2 u |xn| for the sum x + step; |g_h| / Delta for alpha; |predicted|).  The iteration feeds alpha back, so c has
             no closed form: it is 4 x the worst distance of the host's float64 restatement (trf_step_f64, NOT the device) from
             the long-double one over the committed cases, c = 14.7 (worst ratio 3.67, alpha of a 9-parameter model case;
             computed and asserted by tests/test_fit_step_host.py, stored in the fixture).  The device's fma / rsqrt-reciprocal
             forms differ from numpy's divisions by a few ulp per operation, the same order.
  invariants on every case, breakdown included: everything finite, |step_h| <= Delta (1 + 8 u), lb < xn < ub strictly,
             branch 1: step = s d p_h with one 0 < s <= 1, branch 3: step_h = -s g_h with one s > 0.

Teeth (verified on the host by injecting each error into trf_step_f64, tests/test_fit_step_host.py::test_injected_errors_are_seen;
case numbers count through the fixture): the reflection flipping the wrong components, or the other root of the trust-region
intersection, changes the branch on 46 cases (first 9, 10, 11, 12); theta on to_tr instead of to_bound moves step / step_h /
predicted beyond the bar on 7 cases (83, 121, 124, 130, 166, 218, ...); the rank threshold with m = N flips the full-rank flag on
the three tiny-column rank_edge cases with m > N (108, 112, 192); alpha_in without the Delta / Delta_new rescaling (what
`alpha *= Delta / Delta_new` in trf_solve feeds the next step; the probe cannot run that line itself) moves alpha / p_h / step_h
beyond the bar on 17 warm-start cases (60, 63, 70, ...).

The `breakdown` class (10 cases, P = 7, 9, 11, from the model at over-parameterised orders): after the 10th pass the update leaves
alpha NEGATIVE (scipy's iteration does the same: same alpha, same 10 passes) and the final factorisation of B + alpha I, which is
then indefinite, meets a non-positive pivot.  scipy's SVD form evaluates -(B + alpha I)^-1 g_h for the indefinite matrix all the
same, and so does solve_tr: its last solve goes through an L D L^T factorisation (ldl_solveN) when the Cholesky one fails.
test_breakdown_cases_against_scipy holds the device to scipy's step there (c kappa u, kappa of the indefinite B + alpha I) and
prints the table.  Before that solve existed, the factor with cholN's substituted pivots (1.0) was used, and this test failed on 4
of the 10 cases (MI355X; the host's float64 restatement gave the same figures): case 197 (n = 9) |step_h - scipy| = 0.524 Delta,
predicted -30.77 against 4.054; case 237 (n = 11) 0.996 Delta, -2894 against 2152; case 239 (n = 11) 0.962 Delta, 6.935e6
against 8.449e6; case 240 (n = 11) 3.1e-4 Delta against a bar of 2e-8.  Decisive cases on MI355X: worst ratio to the bar's unit
2.95 (alpha, n = 11), B within 4.11 u; per order in docs/EXPERIMENTS.md section 31.
"""
import numpy as np
import pytest

from conftest import golden
import sr_oracle as o

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ORDERS = (2, 3, 4, 5, 7, 9, 11)


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def fixture():
    return golden('fit_step_cases.npz')


@pytest.fixture(scope='module')
def cases(fixture):
    """per order: [(fixture index, case, class, long-double step)]"""
    out = {P: [] for P in ORDERS}
    for i, (case, cls) in enumerate(o.step_cases(fixture)):
        out[case[0].size].append((i, case, cls, o.trf_step_exact(*case)))
    return out


@pytest.fixture(scope='module')
def device(ctx, cases):
    """per order: the probe's outputs per case.  tau_max is one kernel argument, so all cases of an order that share it go in one
    launch (a handful per order), rows put back in the fixture's order"""
    out = {}
    for P, cs in cases.items():
        x, A, g = (np.array([c[1][k] for c in cs]) for k in range(3))
        dev = [None] * len(cs)
        for tm in sorted({c[1][3] for c in cs}):
            idx = [k for k, c in enumerate(cs) if c[1][3] == tm]
            r = ctx.expfit_step_probe(x[idx], A[idx], g[idx], [cs[k][1][5] for k in idx], [cs[k][1][6] for k in idx],
                                      [cs[k][1][4] for k in idx], tm)
            for j, k in enumerate(idx):
                dev[k] = {key: val[j] for key, val in r.items()}
        out[P] = dev
    return out


def f64(a):
    return np.asarray(a, dtype=np.float64)


def rel_err(dev, ex):
    ex = np.asarray(ex, dtype=np.longdouble)
    err = np.abs(np.asarray(dev, dtype=np.longdouble) - ex)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.max(np.where(ex != 0, err / np.abs(ex), np.where(err == 0, 0, np.inf))))


@pytest.mark.parametrize('P', ORDERS)
def test_step_against_long_double(P, cases, device, fixture):
    c = float(fixture['c_bar'])
    worst = {}
    for (i, case, cls, ex), dev in zip(cases[P], device[P]):
        if cls == 'breakdown':
            continue
        tag = (i, cls)
        assert dev['pivot_failures'] == 0, tag
        assert np.array_equal(dev['dv'], f64(ex['dv'])), tag
        assert dev['branch'] == ex['branch'] and dev['full_rank'] == ex['full_rank'] and dev['iterations'] == ex['iterations'], \
            (tag, dev['branch'], ex['branch'], dev['full_rank'], ex['full_rank'], dev['iterations'], ex['iterations'])
        assert np.array_equal(np.sign(dev['step_h']), np.sign(f64(ex['step_h']))), tag
        for key, k_u in (('v', 1), ('d', 2), ('g_h', 3), ('B', 7), ('g_norm', 2)):
            r = rel_err(dev[key], ex[key]) / U
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= k_u, (tag, key, r)
        th = abs(dev['theta'] - float(ex['theta'])) / U
        assert th <= 2 * float(ex['g_norm']) + 1, (tag, th)
        ratios = o.step_ratios(ex, dev)
        for key, r in ratios.items():
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= c, (tag, key, r, o.step_kappa(ex['B'], ex['alpha']))
        for key in ('step_h_norm', 'step_norm'):
            assert abs(dev[key] - np.linalg.norm(dev[key[:-5]])) <= (P + 2) * U * dev[key], (tag, key)
    print('P=%d worst: %s  (first-layer outputs in u, the others in kappa u scale; bar c = %.3g)' %
          (P, ', '.join('%s %.3g' % kv for kv in sorted(worst.items())), c))


@pytest.mark.parametrize('P', ORDERS)
def test_step_invariants(P, cases, device):
    for (i, case, cls, ex), dev in zip(cases[P], device[P]):
        x, A, g, tau_max, m, Delta, alpha_in = case
        tag = (i, cls)
        lb, ub = o.fit_bounds(P, tau_max)
        for key, val in dev.items():
            assert np.all(np.isfinite(val)), (tag, key)
        assert np.linalg.norm(dev['step_h']) <= Delta * (1 + 8 * U) and dev['step_h_norm'] <= Delta * (1 + 8 * U), tag
        assert np.all(dev['xn'] > lb) and np.all(dev['xn'] < ub), tag
        if dev['branch'] == 1:
            full = dev['d'] * dev['p_h']
            k = int(np.argmax(np.abs(full)))
            s = dev['step'][k] / full[k]
            assert 0 < s <= 1 and np.all(np.abs(dev['step'] - s * full) <= 4 * U * np.abs(s * full)), tag
        if dev['branch'] == 3:
            k = int(np.argmax(np.abs(dev['g_h'])))
            s = -dev['step_h'][k] / dev['g_h'][k]
            assert s > 0 and np.all(np.abs(dev['step_h'] + s * dev['g_h']) <= 4 * U * np.abs(s * dev['g_h'])), tag


@pytest.mark.parametrize('P', ORDERS)
def test_initial_point_and_radius(P, cases, ctx):
    cs = cases[P]
    for tm in sorted({c[1][3] for c in cs}):
        sel = [c for c in cs if c[1][3] == tm]
        # the fixture's points are strictly feasible already: also put every other component on a bound / 1e-11 inside it
        lb, ub = o.fit_bounds(P, tm)
        xs = []
        for k, c in enumerate(sel):
            x = c[1][0].copy()
            if k % 3 == 1:
                x[::2] = np.where(np.arange(P)[::2] % 4 == 0, lb[::2], ub[::2])
            if k % 3 == 2:
                x[1::2] = lb[1::2] + 1e-11 * np.maximum(1.0, ub[1::2])
            xs.append(x)
        g = np.array([c[1][2] for c in sel])
        A = np.array([c[1][1] for c in sel])
        dev = ctx.expfit_step_probe(np.array(xs), A, g, 1.0, 0.0, 50, tm, mode='init')
        for k, c in enumerate(sel):
            ex = o.trf_step_exact(xs[k], A[k], g[k], tm, 50, 0, 0, mode='init')
            f = o.trf_step_f64(xs[k], A[k], g[k], tm, 50, 0, 0, mode='init')
            assert np.array_equal(dev['x'][k], f64(f['x'])), (c[0], dev['x'][k], f64(f['x']))
            assert np.array_equal(dev['dv'][k], f64(ex['dv'])), c[0]
            assert rel_err(dev['v'][k], f['v']) <= U, c[0]
            # the long-double radius belongs to the long-double feasible point; the device's to the float64 one
            exf = o.trf_step_exact(f64(f['x']), A[k], g[k], tm, 50, 0, 0, mode='radius')
            assert abs(dev['Delta'][k] - float(exf['Delta'])) <= (P + 9) * U * float(exf['Delta']), (c[0], dev['Delta'][k], float(exf['Delta']))
    # Delta == 0 -> 1: every component 0 is not feasible, so the rule can only be met through x = 0 made feasible: 1e-10, not 0
    z = ctx.expfit_step_probe(np.zeros((1, P)), np.eye(P)[None], np.ones((1, P)), 1.0, 0.0, 50, 100.0, mode='init')
    assert np.all(z['x'][0] == 1e-10) and z['Delta'][0] > 0


def test_breakdown_cases_against_scipy(cases, device, fixture):
    """After the 10th pass alpha is negative and B + alpha I indefinite (module docstring).  scipy's step is the reference."""
    c = float(fixture['c_bar'])
    rows, bad = [], []
    for P in ORDERS:
        for (i, case, cls, ex), dev in zip(cases[P], device[P]):
            if cls != 'breakdown':
                continue
            sc = o.scipy_step(case, ex)
            Delta = case[5]
            lam = np.linalg.eigvalsh(f64(ex['B'])) + sc['alpha']
            kap = float(np.max(np.abs(lam)) / max(np.min(np.abs(lam)), U * np.max(np.abs(lam))))
            dist = float(np.max(np.abs(dev['step_h'] - sc['step_h'])) / Delta)
            rows.append('case %d P=%d m=%d: pivot failures %d, iterations %d (scipy %d), alpha %.3g (scipy %.3g), branch %d, '
                        '|step_h - scipy| / Delta = %.3g, predicted %.6g (scipy %.6g), kappa %.3g' %
                        (i, P, case[4], dev['pivot_failures'], dev['iterations'], sc['iterations'], dev['alpha'], sc['alpha'],
                         dev['branch'], dist, dev['predicted'], sc['predicted'], kap))
            if not (dist <= c * kap * U and abs(dev['predicted'] - sc['predicted']) <= c * kap * U * abs(sc['predicted'])):
                bad.append(i)
    print('\n'.join(rows))
    assert len(rows) >= 8
    assert not bad, 'device step differs from scipy\'s beyond c kappa u on breakdown cases %r' % bad
