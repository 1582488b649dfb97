"""
GPU tests of the fit kernels' evaluations (kernel 3b, sr_fit.hip) below the level of converged fits.  The solver sees the model,
the residuals and the forward-difference Jacobian only through J^T J, J^T f and the cost; at 7 and 9 parameters the fits are so
ill-conditioned that a noisier evaluation and a harmless change of rounding end in the same spread of outcomes.  So these tests
look at ONE evaluation: sr_expfit_probe_f64 runs Residue::stage, eval_f (point cache included) and eval_jac -- the code k_trf and
k_order_search run -- at a given x, and every output is compared with a high-precision host reference of the same operation
(oracle/sr_oracle.py: expfit_eval_exact, np.longdouble, 80-bit on x86; fd_step_2point, scipy's step rule in float64).

Error bars (u = 2^-53, the unit roundoff of float64).  The device forms e_k = exp(-t/tau_k) either by exp() per point (fit_geo = 0,
or any axis that is not a uniform grid, or L <= 64 W) or, on a uniform grid, by exp() at a thread's first point and one
multiplication per further point of that thread (the points of a thread are NTH = 64 W grid steps apart; j = l // NTH products
since the last exp()).  Per exponential:

    |e_dev - e| <= (c0 + c1 j) u |e| + c2 (t / tau) u |e|   (+ (j + 2) 2^-1074 where results are subnormal)

    exp() per point: c0 = 3 (exp() within 1 ulp, the product C_k e_k), c1 = 0, c2 = 2 (the correctly rounded quotient t / tau);
    products:        c0 = 3, c1 = 3 (each factor exp(-t_step/tau) within 1 ulp, each product rounded), c2 = 12 (the quotients
                     t_0 / tau and t_step / tau, the rounding of t_step, and the grid itself: the axes here are within 1.5 ulp of
                     t_0 + l dt, which moves e by 1.5 u (t / tau) at the point and up to 2 x 1.5 u (t / tau) through t_step).

A residual f = w (S2 + sum C_k e_k - y) adds the rounding of that sum: (K + 3) u w (|S2| + sum |C_k e_k| + |y|) (|S2| -> 1 +
sum |C_k| when S2 = 1 - sum C), plus u |f|.  That per-point bound B(l) is asserted directly on the residuals, and it is what every
other bar is derived from:
  * forward-difference Jacobian: |J_dev - J| <= (B_i(l) + B_0(l)) / |dx_i| + 3 u |J|  (B_i at x + dx_i e_i; the subtraction and
    the shared-divisor division each round once);  analytic Jacobian: the relative bar of e_k, plus 6 u for the tau column;
  * J^T J, J^T f, cost: the first-order propagation of those per-point bars, sum_l (D_il |J_jl| + |J_il| D_jl + D_il D_jl), plus
    the reduction's own rounding gamma sum_l |J_il J_jl| with gamma = (ceil(L / NTH) + W + 8) u (a thread's sequential fma
    chain, six butterfly levels across a wave, W - 1 additions across waves).
Errors of J^T J are reported scaled by sqrt(A_ii A_jj); the assertions are element-wise against the derived bars.
"""
import numpy as np
import pytest

from conftest import golden
import sr_oracle as o

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TINY = 2.0 ** -1074
EXP_C = (3.0, 0.0, 2.0)          # (c0, c1, c2): exp() per point
GEO_C = (3.0, 3.0, 12.0)         # products along a thread's points
ORDERS = (2, 3, 5, 7, 9)
WAVES = (1, 2, 4)
# slow components: the products' J^T J deviation from exact <= this x that of exp() per point (test_probe_vs_high_precision_reference).
# Not derived -- the exp()-per-point deviation has no lower bound to derive a ratio from -- but stated: measured on MI355X over the
# sweep up to 61 / 11.0 / 8.7 (W = 1 / 2 / 4); the bar leaves ~35 % above that, so a longer chain or a noisier factor shows up.
SLOW_FACTOR = {1: 80.0, 2: 15.0, 4: 12.0}


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.set_option('fit_waves', 2)
    c.set_option('fit_lds', 1)
    c.set_option('fit_geo', 1)
    c.close()


def _bounds(n, tau_max):
    K = n // 2
    lb = np.zeros(n)
    ub = np.ones(n)
    ub[K:2 * K] = tau_max
    return lb, ub


def point_bound(t, y, w, x, e, NTH, geo, f):
    """B(l): bound on |f_dev(l) - f(l)| (module docstring).  e: the exact exponentials at x (K, L); f: exact residuals."""
    n = x.size
    K = n // 2
    L = t.size
    c0, c1, c2 = GEO_C if geo else EXP_C
    j = (np.arange(L) // NTH).astype(np.float64) if geo else np.zeros(L)
    C = np.abs(x[:K])
    a = C[:, None] * np.asarray(e, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        q = np.abs(t)[None, :] / x[K:2 * K, None]
        rel = (c0 + c1 * j)[None, :] + c2 * q
    exp_part = np.sum(np.where(a > 0, rel * a, 0.0), axis=0)
    S2abs = abs(x[-1]) if n % 2 else 1.0 + np.sum(C)
    sum_part = (K + 3) * (S2abs + np.sum(a, axis=0) + np.abs(y))
    under = (j + 2) * TINY * (np.sum(C) + 1.0) * 4
    return w * (U * (exp_part + sum_part) + under) + U * np.abs(np.asarray(f, dtype=np.float64))


def exp_rel_bound(t, x, e, NTH, geo):
    """relative bar of e_k (K, L) and its absolute floor for subnormal results"""
    K = x.size // 2
    c0, c1, c2 = GEO_C if geo else EXP_C
    L = t.size
    j = (np.arange(L) // NTH).astype(np.float64) if geo else np.zeros(L)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        q = np.abs(t)[None, :] / x[K:2 * K, None]
        rel = np.where(np.asarray(e, dtype=np.float64) > 0, ((c0 + c1 * j)[None, :] + c2 * q) * U, 0.0)
    return rel, (j + 2)[None, :] * TINY * 4


def derived_bars(t, y, w, x, ref, NTH, W, geo, jac_mode):
    """Bars for the probe's outputs at x: (B0 per point, D (L, n) per Jacobian element, bar_A (n, n), bar_g (n), bar_cost)."""
    n = x.size
    K = n // 2
    L = t.size
    lb, ub = _bounds(n, np.inf)
    f0 = np.asarray(ref['f'], dtype=np.float64)
    J = np.asarray(ref['J'], dtype=np.float64)
    B0 = point_bound(t, y, w, x, ref['e'], NTH, geo, f0)
    D = np.empty((L, n))
    if jac_mode == 0:
        h = ref['dx_h'][0]
        for i in range(n):
            xi = x.copy()
            xi[i] = x[i] + h[i]
            Bi = point_bound(t, y, w, xi, ref['ei'][i], NTH, geo, ref['fi'][i])
            D[:, i] = (Bi + B0) / abs(ref['dx'][i]) + 3 * U * np.abs(J[:, i])
    else:
        rel, floor = exp_rel_bound(t, x, ref['e'], NTH, geo)
        e = np.asarray(ref['e'], dtype=np.float64)
        for k in range(K):
            D[:, k] = w * (rel[k] * e[k] + floor[0] + 2 * U * (np.abs(e[k]) + 1.0))
            with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
                tfac = np.abs(x[k]) * np.abs(t) / (x[K + k] * x[K + k])
            D[:, K + k] = np.abs(J[:, K + k]) * (rel[k] + 6 * U) + w * tfac * floor[0] + TINY
        if n % 2:
            D[:, n - 1] = 0.0
    gam = (int(np.ceil(L / NTH)) + W + 8) * U * 1.01
    aJ = np.abs(J)
    bar_A = D.T @ aJ + aJ.T @ D + D.T @ D + gam * ((aJ + D).T @ (aJ + D))
    af = np.abs(f0)
    bar_g = D.T @ af + aJ.T @ B0 + D.T @ B0 + gam * ((aJ + D).T @ (af + B0))
    bar_cost = np.sum(af * B0 + 0.5 * B0 * B0) + gam * 0.5 * np.sum((af + B0) ** 2)
    return B0, D, bar_A, bar_g, bar_cost


def grid_axis(L, t0, dt):
    return t0 + dt * np.arange(L, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# the cases: (name, t (L), y (R, L), sigma (R, L) or None, x (R, n), tau_max) for one number of parameters n
# ------------------------------------------------------------------------------------------------------------------------
def _synthetic_x(n, t, tau_max, rng):
    """tau from below dt to tau_max = 10 t_max; x on the bounds (C = 0 / 1, S2 = 0 / 1, tau = tau_max); x where x + h leaves the
    box (C, S2 within h of 1, tau within h of tau_max: scipy then steps backwards)."""
    K = n // 2
    dt = t[1] - t[0]
    rows = []
    for r in range(6):
        C = rng.uniform(0.02, 0.9 / K, K)
        taus = np.exp(rng.uniform(np.log(0.3 * dt), np.log(tau_max), K))
        S2 = rng.uniform(0.05, 0.9)
        if r == 1:
            taus[-1] = tau_max                          # on the upper bound
            C[0] = 0.0                                  # on the lower bound
        if r == 2:
            taus = np.geomspace(0.5 * dt, tau_max * (1 - 1e-10), K)   # x + h > tau_max: backward step
            C[-1] = 1.0 - 1e-9 if K == 1 else C[-1]
        if r == 3:
            taus = np.geomspace(t[-1], tau_max, K)       # slow components only (tau >= t_max)
        if r == 4:
            S2 = 1.0 if n % 2 else S2                   # S2 on its upper bound
            taus[0] = 0.3 * dt                          # faster than one sample
        if r == 5:
            S2 = 0.0
            C = np.full(K, 1.0 / K) if K > 1 else np.array([1.0])
        x = np.concatenate([C, taus] + ([[S2]] if n % 2 else []))
        rows.append(x)
    return np.array(rows)


def _model_data(t, x, rng, noise=2e-4):
    out = np.empty((x.shape[0], t.size))
    for i in range(x.shape[0]):
        out[i] = o.curvefit_exponential(t, *x[i]) + noise * rng.standard_normal(t.size)
    return out


LENGTHS = (64, 65, 128, 129, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048, 2049)


def _cases(n):
    rng = np.random.default_rng(100 + n)
    cases = []
    # the reference's own inputs: p0 and popt of every residue of the fixtures (cfg2 L = 512, cfg3s L = 2048; t = 10 (1..L))
    for tag in ('cfg2', 'cfg3s'):
        g = golden('%s_fit.npz' % tag)
        j = list(g['listDoG']).index(n)
        rows = slice(0, 6)
        t = g['t'][0]
        assert np.all(g['t'] == t)
        x = np.concatenate([g['trial_p0'][rows, j, :n], np.nan_to_num(g['trial_popt'][rows, j, :n], nan=0.5)])
        ok = np.all(np.isfinite(x), axis=1) & np.all(x[:, n // 2:2 * (n // 2)] > 0, axis=1)
        x = x[ok]
        y = np.concatenate([g['y'][rows], g['y'][rows]])[ok]
        dy = np.concatenate([g['dy'][rows], g['dy'][rows]])[ok]
        cases.append(('%s' % tag, t, y, dy, x, t[-1] * 10))
    # synthetic: every length around the thread counts and the point-cache edge 8 NTH, shifted origins, with / without sigma
    for m, L in enumerate(LENGTHS):
        t0, dt = ((0.0, 10.0), (10.0, 10.0), (3.5, 2.0))[m % 3]
        t = grid_axis(L, t0, dt)
        tau_max = 10 * t[-1]
        x = _synthetic_x(n, t, tau_max, rng)
        y = _model_data(t, x, rng)
        dy = None if m % 2 else np.full_like(y, 1e-3) * (1 + 0.1 * np.sin(np.arange(L)))[None, :]
        cases.append(('L%d_t0%g' % (L, t0), t, y, dy, x, tau_max))
    return cases


def _exact(case, jac_mode):
    name, t, y, dy, x, tau_max = case
    lb, ub = _bounds(x.shape[1], tau_max)
    out = []
    for i in range(x.shape[0]):
        w = np.ones(t.size) if dy is None else 1.0 / dy[i]
        r = o.expfit_eval_exact(t, y[i], w, x[i], lb, ub, jac_mode)
        r['dx_h'] = o.fd_step_2point(x[i], lb, ub)
        r['w'] = w
        out.append(r)
    return out


def _probe(ctx, case, W, lds, geo, jac_mode):
    name, t, y, dy, x, tau_max = case
    ctx.set_option('fit_waves', W)
    ctx.set_option('fit_lds', lds)
    ctx.set_option('fit_geo', geo)
    return ctx.expfit_probe(t[None, :], y, dy, x, tau_max, jac_mode)


def _scaled(err, A):
    d = np.sqrt(np.abs(np.diag(A)))
    s = np.outer(d, d)
    return np.max(np.where(s > 0, err / np.where(s > 0, s, 1), 0.0))


@pytest.mark.parametrize('n', ORDERS)
def test_probe_vs_high_precision_reference(ctx, n):
    """Every (W, fit_lds, fit_geo, jac_mode) at every length of LENGTHS and on the fixtures' p0 / popt, n parameters:
      * dx is bit-identical to scipy's step rule (oracle fd_step_2point; x on the bounds, x + h outside the box included);
      * the uniform-grid flag is set exactly when fit_geo = 1 and L > 64 W (every axis here is a uniform grid, t_0 = 0, 10, 3.5);
      * fit_geo = 0 (exp() per point): the residuals are BIT-IDENTICAL to sr_expfit_resjac_f64 (k_resjac: IEEE division and the
        library exp()) -- the shared-divisor division and the fused exp sequence give the same bits as exp(a / b);
      * the residuals are within B(l) of the 80-bit reference, J^T J / J^T f / cost within the bars derived from B (module
        docstring), for the products (c1 = 3 per product since the last exp()) at every W and for exp() per point;
      * fit_lds = 0 and 1 give bit-identical outputs (the data moves, the arithmetic does not);
      * slow components (every tau >= t_max, jac_mode 0): the products' relative deviation of the tau diagonal of J^T J from exact,
        root-mean-square over the cases, is at most SLOW_FACTOR[W] times that of exp() per point on the same inputs.  This is where
        the chain costs accuracy: a slow component's forward difference is a small difference of two long product chains, so
        its Jacobian is up to 11 times noisier than with exp() per point at W = 2 (15 products at L = 2048), 9 at W = 4 (7
        products), 61 at W = 1 (31 products) -- still within the derived bars above."""
    worst = {}
    slow = {W: [[], []] for W in WAVES}
    for case in _cases(n):
        name, t, y, dy, x, tau_max = case
        L = t.size
        resid_ref, _ = ctx.expfit_resjac(np.broadcast_to(t, y.shape), y, dy, x, want_jac=False)
        for jac_mode in (0, 1):
            ref = _exact(case, jac_mode)
            for W in WAVES:
                NTH = 64 * W
                per_geo = {}
                for geo in (1, 0):
                    outs = [_probe(ctx, case, W, lds, geo, jac_mode) for lds in (1, 0)]
                    for key in outs[0]:
                        assert np.array_equal(outs[0][key], outs[1][key], equal_nan=True), (name, W, geo, jac_mode, key)
                    p = outs[0]
                    per_geo[geo] = p
                    assert np.all(p['geo'] == (1 if (geo and L > NTH) else 0)), (name, W, geo, p['geo'])
                    if geo == 0:
                        assert np.array_equal(p['f'], resid_ref), (name, W, jac_mode)
                    for i in range(x.shape[0]):
                        r = ref[i]
                        assert np.array_equal(p['dx'][i], r['dx']), (name, i, p['dx'][i], r['dx'])
                        B0, D, bar_A, bar_g, bar_cost = derived_bars(t, y[i], r['w'], x[i], r, NTH, W, p['geo'][i], jac_mode)
                        ef = np.abs(p['f'][i] - np.asarray(r['f'], dtype=np.float64))
                        A_ref = np.asarray(r['JtJ'], dtype=np.float64)
                        eA = np.abs(p['JtJ'][i] - A_ref)
                        eg = np.abs(p['Jtf'][i] - np.asarray(r['Jtf'], dtype=np.float64))
                        ec = abs(p['cost'][i] - float(r['cost']))
                        key = (W, int(p['geo'][i]), jac_mode)
                        wk = worst.setdefault(key, [0.0, 0.0, 0.0])
                        wk[0] = max(wk[0], float(np.max(ef / B0)))
                        wk[1] = max(wk[1], float(np.max(np.where(bar_A > 0, eA / bar_A, 0))))
                        wk[2] = max(wk[2], _scaled(eA, A_ref))
                        ctxt = (name, i, W, geo, jac_mode)
                        assert np.all(ef <= B0), (ctxt, 'f', float(np.max(ef / B0)))
                        assert np.all(eA <= bar_A), (ctxt, 'JtJ', float(np.max(eA / np.maximum(bar_A, 1e-300))))
                        assert np.all(eg <= bar_g), (ctxt, 'Jtf', float(np.max(eg / np.maximum(bar_g, 1e-300))))
                        assert ec <= bar_cost, (ctxt, 'cost', ec, bar_cost)
                if jac_mode == 0 and L > NTH:
                    K = n // 2
                    for i in range(x.shape[0]):
                        if np.all(x[i, K:2 * K] >= t[-1]):
                            A_ref = np.asarray(ref[i]['JtJ'], dtype=np.float64)
                            dA = np.diag(A_ref)[K:2 * K]
                            use = dA > 0                    # (a component with C = 0 has a zero tau column)
                            for geo in (1, 0):
                                e = np.abs(np.diag(per_geo[geo]['JtJ'][i])[K:2 * K] - dA)
                                slow[W][geo].append(e[use] / dA[use])
    print('\n[probe n=%d] (W, geo, jac_mode): worst |f - f_ref| / B, worst |JtJ - ref| / bar, worst scaled JtJ error' % n)
    for k in sorted(worst):
        print('   %s: %.2f  %.2f  %.1e' % (k, *worst[k]))
    rms = {}
    for W in WAVES:
        rms[W] = [float(np.sqrt(np.mean(np.concatenate(slow[W][geo]) ** 2))) for geo in (1, 0)]
        print('   slow components, W=%d: rms relative tau-diagonal error of J^T J, products %.2e, exp() per point %.2e (ratio %.2f)'
              % (W, rms[W][0], rms[W][1], rms[W][0] / max(rms[W][1], 1e-300)))
    for W in WAVES:
        assert rms[W][0] <= SLOW_FACTOR[W] * rms[W][1], (n, W, rms[W])


def test_exp_per_point_bits_over_a_tau_sweep(ctx):
    """exp() per point (fit_geo = 0) against k_resjac's exp((-t) / tau) bit for bit over taus that stress the shared-divisor
    division and the fused exp sequence: significands of all ones (the case Markstein's theorem leaves open), quotients between
    -708 and -745 (subnormal results) and below -745 (zero), t = 0, the smallest subnormal tau (what strictly_feasible's
    nextafter(0, ub) makes of a tau on its lower bound: 1 / tau overflows) and other taus whose reciprocal overflows.  The product
    path (fit_geo = 1) on the same inputs: within B(l) of the 80-bit reference -- at t = 0 the seed exp(-0 / tau) = 1 as well."""
    rng = np.random.default_rng(7)
    L = 1500
    t = grid_axis(L, 0.0, 10.0)
    t_max = t[-1]
    taus = [np.nextafter(2.0 ** k, 0) for k in (-2, 0, 3, 7, 10, 12, 14, 16, 17, 19)]
    taus += [t_max / 720.0, t_max / 740.0, t_max / 744.5, t_max / 708.5, t_max / 760.0, t_max / 5000.0]
    taus += [5e-324, 2.0 ** -1030, 2.0 ** -1024 * 0.75, 1e-300, 3.0, 7.0, 9.999999999999998, 1.0 / 3.0]
    taus = np.array(taus)
    for n in (3, 2, 5):
        K = n // 2
        tau_max = max(10 * t_max, taus.max())
        x = []
        for i in range(0, taus.size, K):
            tk = taus[i:i + K]
            if tk.size < K:
                tk = np.concatenate([tk, taus[:K - tk.size]])
            C = rng.uniform(0.05, 0.9 / K, K)
            x.append(np.concatenate([C, tk] + ([[0.3]] if n % 2 else [])))
        x = np.array(x)
        y = np.full((x.shape[0], L), 0.5)
        lb, ub = _bounds(n, tau_max)
        resid, _ = ctx.expfit_resjac(np.broadcast_to(t, y.shape), y, None, x, want_jac=False)
        assert np.all(np.isfinite(resid))
        for W in WAVES:
            for geo in (0, 1):
                ctx.set_option('fit_waves', W)
                ctx.set_option('fit_geo', geo)
                ctx.set_option('fit_lds', 1)
                p = ctx.expfit_probe(t[None, :], y, None, x, tau_max, 0)
                if geo == 0:
                    bad = np.argwhere(p['f'] != resid)
                    assert bad.size == 0, (n, W, [(int(i), int(l), x[i], t[l], p['f'][i, l], resid[i, l]) for i, l in bad[:4]])
                for i in range(x.shape[0]):
                    f, e = o.expfit_residuals_ld(t, y[i], np.ones(L), x[i])
                    B = point_bound(t, y[i], np.ones(L), x[i], e, 64 * W, p['geo'][i], f)
                    err = np.abs(p['f'][i] - np.asarray(f, dtype=np.float64))
                    assert np.all(err <= B), (n, W, geo, i, x[i], int(np.argmax(err / B)), float(np.max(err / B)))
    ctx.set_option('fit_waves', 2)
    ctx.set_option('fit_geo', 1)


def test_uniform_grid_detection(ctx):
    """Residue::stage's decision, per residue and for every W: the products are taken for t_0 + dt * arange(L) (within 1.5 ulp
    of the grid; t_0 = 0, 10, 3.5) when L > 64 W, and NOT for an axis with one time moved by 9 ulp (at a point j >= 1 of its
    thread, where 9 ulp exceed the 1.8e-15 relative threshold), a decreasing axis, L <= 64 W, a quadratic axis.  Where the flag is
    off the outputs are bit-identical to fit_geo = 0."""
    L = 1000
    n = 3
    x = np.array([[0.3, 500.0, 0.6]])
    base = {t0: grid_axis(L, t0, 10.0) for t0 in (0.0, 10.0, 3.5)}
    moved = base[0.0].copy()
    moved[410] = moved[410] + 9 * np.spacing(moved[410])             # 4100: just above 2^12, ulp / t = 2.2e-16
    assert abs(moved[410] - base[0.0][410]) > 1.8e-15 * moved[410]
    axes = [('grid t0=%g' % t0, tt, True) for t0, tt in base.items()]
    axes += [('moved 9 ulp', moved, False), ('decreasing', base[10.0][::-1].copy(), False),
             ('quadratic', base[10.0] * (1 + 1e-3 * base[10.0] / base[10.0][-1]), False)]
    for W in WAVES:
        NTH = 64 * W
        short = grid_axis(NTH, 10.0, 10.0)
        for name, t, want in axes + [('L = NTH', short, False)]:
            y = 0.6 + 0.3 * np.exp(-t / 500.0)[None, :]
            out = {}
            for geo in (1, 0):
                ctx.set_option('fit_waves', W)
                ctx.set_option('fit_geo', geo)
                out[geo] = ctx.expfit_probe(t[None, :], y, None, x, 10 * np.max(t), 0)
            assert out[1]['geo'][0] == (1 if want else 0), (W, name)
            assert out[0]['geo'][0] == 0
            if not want:
                for k in out[1]:
                    if k != 'geo':
                        assert np.array_equal(out[1][k], out[0][k]), (W, name, k)
    ctx.set_option('fit_waves', 2)
    ctx.set_option('fit_geo', 1)


@pytest.mark.parametrize('tag', ['cfg2', 'cfg3s'])
def test_order_search_lds_on_off_bit_identical(ctx, tag):
    """The model-order search on the fixtures with the residue staged in LDS (fit_lds = 1) and read from global memory
    (fit_lds = 0, Residue<W, false>): bit-identical selections, parameters, chi^2 and evaluation counts, at every W."""
    from spinrelax_amd import fitting_Ct_functions as fitCt
    g = golden('%s_fit.npz' % tag)
    t, y, dy = g['t'], g['y'], g['dy']
    orders = tuple(int(v) for v in g['listDoG'])
    try:
        for W in (2, 4, 1) if tag == 'cfg2' else (2,):
            ctx.set_option('fit_waves', W)
            res = []
            for lds in (1, 0):
                ctx.set_option('fit_lds', lds)
                res.append(fitCt.order_search_device(t, y, dy, orders, 0.5, ctx=ctx))
            for k in res[0]:
                assert np.array_equal(np.asarray(res[0][k]), np.asarray(res[1][k]), equal_nan=True), (tag, W, k)
    finally:
        ctx.set_option('fit_lds', 1)
        ctx.set_option('fit_waves', 2)
