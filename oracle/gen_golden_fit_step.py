#!/usr/bin/env python3
"""
gen_golden_fit_step.py -- cases for ONE trust-region step of the device fit (sr_expfit_step_probe_f64).

TEST INFRASTRUCTURE:   python oracle/gen_golden_fit_step.py        (CPU only, a few minutes; deterministic)

Writes tests/golden/fit_step_cases.npz: per order P in ORDERS the inputs of the step probe (x, A = J^T J, g = J^T f, tau_max, m,
Delta, alpha_in), the class of each case and, for the warm-start cases, the (alpha, Delta) of the step before.  Data only; the
expected outputs are computed by the tests from oracle/sr_oracle.py (trf_step_exact).

Classes:
  model      A, g from the oracle's exact evaluation (expfit_eval_exact, 2-point Jacobian) of the multi-exponential model on the
             decays of cfg1 (L = 50), cfg2 (first 300 points) and cfg3s (L = 2048), with and without sigma, at the reference's own
             trial_p0 / trial_popt, at random feasible points, and with components pushed to 1e-12 .. 1e-3 of a bound (1e-10 is
             exactly the point strictly_feasible(., 1e-10) makes); Delta = 1e-6 .. 3 times the initial radius; alpha_in = 0 or the
             alpha of a step before at another radius, rescaled as trf_solve rescales it
  synthetic  random symmetric positive definite A with a log-uniform spectrum, random x and g: fills the branch quotas the model
             cases leave open (reflected steps at P = 2, 3 are about 1 in 400 random cases)
  edge       constructed: a gradient component exactly 0, a tie in `hits`, a step component exactly 0, g_norm on both sides of
             0.005
  rank_edge  duplicated / nearly duplicated columns and a tiny uncoupled column on either side of (EPS m)^2 max diag; built from
             small integers and powers of two, so that the pivots are exact in float64 and in long double alike
  breakdown  float64 meets a non-positive pivot of B + alpha I inside the alpha iteration (trf_step_f64 says so)
Every case outside `breakdown` is DECISIVE: each decision margin of trf_step_exact is >= MARGIN (rank_edge: all but the pivot
margins, whose arithmetic is exact by construction) and trf_step_f64 takes the same decisions.  The search runs until every
select_step branch, and both solve_tr outcomes of branch 0, occur QUOTA times per order.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sr_oracle as o                               # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
ORDERS = (2, 3, 4, 5, 7, 9, 11)
CLASSES = ('model', 'synthetic', 'edge', 'rank_edge', 'breakdown')
MARGIN = 1e-6
BUCKETS = ('b0_alpha0', 'b0_alpha', 'b1', 'b2', 'b3')
EVENTS = ('alpha_clamped', 'iterations_exhausted', 'hits_tie', 'zero_step_component', 'r_value_inf', 'cauchy_to_bound')
U = 2.0 ** -53


def quota(P):
    return 6 if P >= 5 else 3


def keep_per_bucket(P):
    return 7 if P >= 5 else 4


def bucket(r):
    if r['branch'] == 0:
        return 'b0_alpha0' if r['alpha'] == 0 else 'b0_alpha'
    return 'b%d' % r['branch']


DISCRETE = ('branch', 'full_rank', 'iterations', 'pivot_failures')


def same_decisions(a, b):
    return all(a[k] == b[k] for k in DISCRETE) and np.array_equal(np.asarray(a['dv'], dtype=float), np.asarray(b['dv'], dtype=float)) \
        and np.array_equal(np.sign(np.asarray(a['step_h'], dtype=float)), np.sign(np.asarray(b['step_h'], dtype=float))) \
        and a['events'] == b['events']


def decisive(case, cls='model'):
    """(exact result, float64 result) when the case is decisive, else None."""
    ex = o.trf_step_exact(*case)
    marg = dict(ex['margins'])
    if cls == 'rank_edge':
        marg.pop('rank', None)
        marg.pop('pivot', None)
    if ex['pivot_failures'] or not all(np.isfinite(np.asarray(ex[k], dtype=float)).all() for k in ('step', 'step_h', 'predicted', 'xn')):
        return None
    if min(marg.values()) < MARGIN:
        return None
    f = o.trf_step_f64(*case)
    if not same_decisions(ex, f):
        return None
    return ex, f


def load_decays():
    out = []
    for tag, L in (('cfg1', 50), ('cfg2', 300), ('cfg3s', 2048)):
        g = np.load(os.path.join(GOLD, '%s_fit.npz' % tag), allow_pickle=True)
        out.append(dict(t=g['t'][:, :L], y=g['y'][:, :L], dy=g['dy'][:, :L], orders=[int(n) for n in g['listDoG']],
                        p0=g['trial_p0'], popt=g['trial_popt']))
    return out


def feasible(x, tau_max):
    lb, ub = o.fit_bounds(x.size, tau_max)
    return np.array(o._strictly_feasible(np.float64, list(x), list(lb), list(ub), 1e-10), dtype=np.float64)


def model_point(rng, decays, P):
    """x, A, g, tau_max, m at a point of the model."""
    dc = decays[rng.randint(len(decays))]
    i = rng.randint(dc['t'].shape[0])
    t, y, dy = dc['t'][i], dc['y'][i], dc['dy'][i]
    w = 1.0 / dy if rng.rand() < 0.5 else np.ones_like(y)
    tau_max = 10.0 * t[-1]
    K = P // 2
    lb, ub = o.fit_bounds(P, tau_max)
    kind = rng.randint(3)
    x = None
    if kind < 2 and P in dc['orders']:
        src = (dc['p0'], dc['popt'])[kind][i, dc['orders'].index(P), :P]
        if np.all(np.isfinite(src)) and np.all(src >= lb) and np.all(src <= ub):
            x = np.array(src, dtype=np.float64)
    if x is None:
        x = np.concatenate([rng.rand(K) / K, np.exp(rng.uniform(np.log(t[0]), np.log(tau_max), K)), rng.rand(P % 2)])
    if rng.rand() < 0.5:
        for j in rng.choice(P, size=1 + rng.randint(2), replace=False):
            e = (1e-12, 1e-10, 1e-8, 1e-6, 1e-4, 1e-3)[rng.randint(6)]
            x[j] = lb[j] + e * max(1.0, abs(lb[j])) if rng.rand() < 0.5 else ub[j] - e * max(1.0, abs(ub[j]))
    x = feasible(x, tau_max)
    ev = o.expfit_eval_exact(t, y, w, x, lb, ub, 0)
    A = np.asarray(ev['JtJ'], dtype=np.float64)
    return x, 0.5 * (A + A.T), np.asarray(ev['Jtf'], dtype=np.float64), tau_max, t.size


def synthetic_point(rng, P):
    tau_max = (20.0, 500.0, 20480.0)[rng.randint(3)]
    lb, ub = o.fit_bounds(P, tau_max)
    x = lb + (ub - lb) * rng.rand(P)
    for j in range(P):
        if rng.rand() < 0.4:
            e = 10.0 ** rng.uniform(-6, -1)
            x[j] = lb[j] + e * (ub[j] - lb[j]) if rng.rand() < 0.5 else ub[j] - e * (ub[j] - lb[j])
    Q, _ = np.linalg.qr(rng.randn(P, P))
    A = (Q * 10.0 ** rng.uniform(-rng.uniform(0, 8), 0, P)) @ Q.T
    s = 1.0 / np.sqrt(np.maximum(x - lb, ub - x))
    A = A * np.outer(s, s)
    g = rng.randn(P) * np.sqrt(np.diag(A)) * 10.0 ** rng.uniform(-3, 1)
    return feasible(x, tau_max), 0.5 * (A + A.T), g, tau_max, (50, 300, 2048)[rng.randint(3)]


def radii(rng, x, A, g, tau_max, m):
    """(Delta, alpha_in, alpha_prev, Delta_prev) tuples: cold starts and one warm start."""
    D0 = float(o.trf_step_f64(x, A, g, tau_max, m, 0, 0, mode='init')['Delta'])
    out = [(D0 * 10.0 ** rng.uniform(-6, np.log10(3.0)), 0.0, 0.0, 0.0) for _ in range(3)]
    out.append((D0 * 3.0, 0.0, 0.0, 0.0))
    Dp = D0 * 10.0 ** rng.uniform(-3, 0)
    prev = o.trf_step_f64(x, A, g, tau_max, m, Dp, 0.0)
    if prev['alpha'] > 0 and np.isfinite(prev['alpha']):
        Dn = (0.25 * float(prev['step_h_norm']), 2.0 * Dp)[rng.randint(2)]
        if Dn > 0:
            out.append((Dn, float(prev['alpha']) * (Dp / Dn), float(prev['alpha']), Dp))     # trf_solve: alpha *= Delta / Delta_new
    return out


class Store:
    def __init__(self):
        self.cases = {P: [] for P in ORDERS}
        self.buckets = {P: {b: 0 for b in BUCKETS} for P in ORDERS}
        self.events = {e: 0 for e in EVENTS}

    def add(self, P, x, A, g, tau_max, m, Delta, alpha, cls, warm=(0.0, 0.0), res=None):
        self.cases[P].append(dict(x=x, A=A, g=g, par=(tau_max, m, Delta, alpha), cls=CLASSES.index(cls), warm=warm))
        if res is not None:
            self.buckets[P][bucket(res)] += 1
            for e in res['events']:
                if e in self.events:
                    self.events[e] += 1

    def total(self):
        return sum(len(v) for v in self.cases.values())


def search_quota(st, rng, decays, P):
    """model cases first; synthetic ones for what they leave open"""
    for cls, tries in (('model', 700 if P >= 5 else 2500), ('synthetic', 20000)):
        for _ in range(tries):
            if all(st.buckets[P][b] >= quota(P) for b in BUCKETS):
                return
            x, A, g, tau_max, m = model_point(rng, decays, P) if cls == 'model' else synthetic_point(rng, P)
            for Delta, alpha, ap, Dp in radii(rng, x, A, g, tau_max, m):
                f = o.trf_step_f64(x, A, g, tau_max, m, Delta, alpha)
                b = bucket(f)
                rare = any(e in EVENTS and st.events[e] < 3 for e in f['events'])
                if f['pivot_failures'] or (st.buckets[P][b] >= keep_per_bucket(P) and not rare):
                    continue
                d = decisive((x, A, g, tau_max, m, Delta, alpha))
                if d is not None:
                    st.add(P, x, A, g, tau_max, m, Delta, alpha, cls, (ap, Dp), d[0])
    raise SystemExit('P=%d: quotas not reached: %r' % (P, st.buckets[P]))


def exhausted_cases(st, rng, want=4):
    """All 10 passes of the alpha iteration used up.  B = diag(lambda) with the eigenvalues a factor of several hundred apart and
    g_h_i = r_i lambda_i: |p(alpha)|^2 = sum (r_i lambda_i / (lambda_i + alpha))^2 is a staircase over 20 to 30 decades of alpha.
    From alpha = 0.001 alpha_upper every Newton step from the right overshoots below alpha_lower, and the restart
    max(0.001 alpha_upper, sqrt(alpha_lower alpha_upper)) only takes three decades at a time."""
    found = 0
    for _ in range(400):
        P = (9, 11)[rng.randint(2)]
        lam = 10.0 ** (-rng.uniform(1.5, 3.2) * np.arange(P))
        rng.shuffle(lam)
        x = rng.uniform(0.5, 0.95, P)                     # g > 0 everywhere: v = x - lb = x
        g = lam * rng.uniform(0.2, 0.5, P) / np.sqrt(x)   # g_h = d g = r lambda
        A = np.diag((lam - g) / x)                        # B = A v + g = diag(lambda)
        Delta = np.sqrt(np.sum((np.sqrt(x) * g / lam) ** 2)) * rng.uniform(0.3, 0.999)
        f = o.trf_step_f64(x, A, g, 2.0, 50, Delta, 0.0)
        if 'iterations_exhausted' in f['events'] and not f['pivot_failures']:
            d = decisive((x, A, g, 2.0, 50, Delta, 0.0))
            if d is not None:
                st.add(P, x, A, g, 2.0, 50, Delta, 0.0, 'synthetic', res=d[0])
                found += 1
                if found == want:
                    return
    raise SystemExit('only %d cases that exhaust the alpha iteration' % found)


def search_events(st, rng):
    """the rarer paths, on synthetic problems, until each has occurred three times"""
    exhausted_cases(st, rng)
    for _ in range(40000):
        need = [e for e in EVENTS if st.events[e] < 3 and e not in ('hits_tie', 'zero_step_component')]
        if not need:
            return
        P = (3, 5, 7)[rng.randint(3)]
        x, A, g, tau_max, m = synthetic_point(rng, P)
        for Delta, alpha, ap, Dp in radii(rng, x, A, g, tau_max, m):
            f = o.trf_step_f64(x, A, g, tau_max, m, Delta, alpha)
            if f['pivot_failures'] or not any(e in need for e in f['events']):
                continue
            d = decisive((x, A, g, tau_max, m, Delta, alpha))
            if d is not None:
                st.add(P, x, A, g, tau_max, m, Delta, alpha, 'synthetic', (ap, Dp), d[0])
    raise SystemExit('events not reached: %r' % st.events)


def edge_cases(st, rng, decays):
    def put(P, x, A, g, tau_max, m, Delta, alpha, cls, want=None):
        d = decisive((x, A, g, tau_max, m, Delta, alpha), cls)
        assert d is not None, (cls, P, want, o.trf_step_exact(x, A, g, tau_max, m, Delta, alpha)['margins'])
        if want:
            assert want(d[0]), (cls, P, d[0]['events'], d[0]['branch'])
        st.add(P, x, A, g, tau_max, m, Delta, alpha, cls, res=d[0])

    for P in (3, 5, 9):
        K = P // 2
        tau_max = 500.0
        # a gradient component exactly 0: v = 1, dv = 0
        for _ in range(200):
            x, A, g, tm, m = model_point(rng, decays, P)
            g = g.copy()
            g[rng.randint(P)] = 0.0
            D0 = float(o.trf_step_f64(x, A, g, tm, m, 0, 0, mode='init')['Delta'])
            if decisive((x, A, g, tm, m, 0.1 * D0, 0.0)) is not None:
                put(P, x, A, g, tm, m, 0.1 * D0, 0.0, 'edge', lambda r: (np.asarray(r['dv'], dtype=float) == 0).any())
                break
        else:
            raise SystemExit('no decisive zero-gradient case at P=%d' % P)
        # uncoupled problem (diagonal A): components 0 and 1 (two amplitudes, same bounds) get the same operations, so they reach
        # the upper bound at exactly the same stride -- a tie in `hits`; component K has g = 0 and no coupling: its step is exactly 0
        # A diagonal but for the coupling of the amplitudes to the last component (S2), whose large gradient drives them over
        # their upper bound (on a diagonal problem the scaled Gauss-Newton step p_i = v_i |g_i| / (A_ii v_i + |g_i|) never
        # leaves the bounds).  P >= 5: amplitudes 0 and 1 are not coupled to each other (L_10 = 0 exactly) and get the same
        # operations in the factorisation and both substitutions, so they reach the bound at exactly the same stride: a tie.
        want = (lambda r: 'hits_tie' in r['events'] and 'zero_step_component' in r['events']) if K > 1 else \
            (lambda r: 'zero_step_component' in r['events'])
        done = False
        for a in (1.0, 2.0, 4.0, 8.0):
            for gc in (1.0, 4.0, 16.0, 64.0):
                for Delta in (0.05, 0.5, 5.0):
                    x = np.concatenate([np.full(K, 0.9), np.full(K, 100.0), np.full(P % 2, 0.5)])
                    A = np.diag(np.concatenate([np.full(K, 3.0), np.full(K, 1e-4), np.full(P % 2, 1.0 + a * a)]))
                    g = np.concatenate([np.full(K, -0.25), np.full(K, 1e-3), np.full(P % 2, gc)])
                    g[K] = 0.0
                    A[:min(K, 2), P - 1] = A[P - 1, :min(K, 2)] = a
                    d = None if done else decisive((x, A, g, tau_max, 50, Delta, 0.0), 'edge')
                    if d is not None and d[0]['branch'] != 0 and want(d[0]):
                        put(P, x, A, g, tau_max, 50, Delta, 0.0, 'edge', want)
                        done = True
        assert done, 'no tie / zero-step case at P=%d' % P
        # g_norm on both sides of 0.005: theta = 0.995 or 1 - g_norm
        x, A, g, tm, m = model_point(rng, decays, P)
        for target in (0.002, 0.0049, 0.0051, 0.5):
            for _ in range(200):
                x, A, g, tm, m = model_point(rng, decays, P)
                r0 = o.trf_step_f64(x, A, g, tm, m, 1.0, 0.0)
                g2 = g * (target / float(r0['g_norm']))
                D0 = float(o.trf_step_f64(x, A, g2, tm, m, 0, 0, mode='init')['Delta'])
                if decisive((x, A, g2, tm, m, 0.3 * D0, 0.0)) is not None:
                    put(P, x, A, g2, tm, m, 0.3 * D0, 0.0, 'edge',
                        lambda r: (float(r['theta']) == 0.995) == (target > 0.005))
                    break
            else:
                raise SystemExit('no decisive g_norm case at P=%d' % P)

    # rank edge: tau components at x = 1 of tau_max = 2 (v = 1 whatever the sign of g), amplitudes with g = 0 (v = 1, dv = 0): B = A + diag(|g|)
    for P, m in ((5, 50), (5, 2048), (9, 300)):
        K = P // 2
        x = np.concatenate([np.full(K, 0.5), np.full(K, 1.0), np.full(P % 2, 0.5)])
        g = np.concatenate([np.zeros(K), np.full(K, 0.5), np.zeros(P % 2)])
        g[K] = -0.25
        T = (o.STEP_EPS * m) ** 2 * 16.0
        for kind in ('duplicate', 'near_duplicate', 'tiny_below', 'tiny_above'):
            A = np.diag(np.concatenate([np.full(K, 4.0), np.full(K, 15.5), np.full(P % 2, 1.0)]))     # B: max diag 16
            A[K, K] = 15.75
            if kind == 'duplicate':
                A[0, 1] = A[1, 0] = 4.0                  # columns 0 and 1 equal: pivot 1 = 4 - 2 * 2 = 0 exactly
            elif kind == 'near_duplicate':
                A[0, 1] = A[1, 0] = 4.0
                A[1, 1] = 4.0 + 2.0 ** -20               # pivot 1 = 2^-20 exactly
            else:
                A[1, 1] = T * (0.5 if kind == 'tiny_below' else 2.0)
            full = kind in ('near_duplicate', 'tiny_above')
            put(P, x, A, g, 2.0, m, 0.01, 0.0, 'rank_edge', lambda r: r['full_rank'] == int(full))


def breakdown_cases(st, rng, decays, want=10):
    """float64 meets a non-positive pivot of B + alpha I in the iteration: over-parameterised model orders near the reference's optimum"""
    found = 0
    for _ in range(6000):
        P = (7, 9, 11, 9)[rng.randint(4)]
        x, A, g, tau_max, m = model_point(rng, decays, P)
        for Delta, alpha, ap, Dp in radii(rng, x, A, g, tau_max, m):
            f = o.trf_step_f64(x, A, g, tau_max, m, Delta, alpha)
            if f['pivot_failures'] and all(np.isfinite(np.asarray(f[k], dtype=float)).all() for k in ('step', 'step_h', 'xn')):
                st.add(P, x, A, g, tau_max, m, Delta, alpha, 'breakdown', (ap, Dp))
                found += 1
                break
        if found >= want:
            return
    raise SystemExit('only %d breakdown cases found' % found)


def main():
    decays = load_decays()
    st = Store()
    for P in ORDERS:
        search_quota(st, np.random.RandomState(1000 + P), decays, P)
        print('P=%d: %d cases, %r' % (P, len(st.cases[P]), st.buckets[P]), flush=True)
    edge_cases(st, np.random.RandomState(77), decays)
    search_events(st, np.random.RandomState(78))
    print('events: %r' % st.events, flush=True)
    breakdown_cases(st, np.random.RandomState(79), decays)
    assert st.total() <= 400, st.total()
    out = dict(orders=np.array(ORDERS), classes=np.array(CLASSES), margin=MARGIN)
    for P in ORDERS:
        cs = st.cases[P]
        out['x_%d' % P] = np.array([c['x'] for c in cs])
        out['A_%d' % P] = np.array([c['A'] for c in cs])
        out['g_%d' % P] = np.array([c['g'] for c in cs])
        out['par_%d' % P] = np.array([c['par'] for c in cs], dtype=np.float64)        # tau_max, m, Delta, alpha_in
        out['cls_%d' % P] = np.array([c['cls'] for c in cs], dtype=np.int8)
        out['warm_%d' % P] = np.array([c['warm'] for c in cs], dtype=np.float64)      # alpha, Delta of the step before (0: cold start)
    # the constant of the conditioning bar: 4 x the worst distance of the float64 restatement from the long-double one, in units
    # of kappa_2(B + alpha I) u (tests/test_fit_step_host.py recomputes and asserts it)
    worst = 0.0
    for case, cls in o.step_cases(out):
        if cls != 'breakdown':
            worst = max(worst, max(o.step_ratios(o.trf_step_exact(*case), o.trf_step_f64(*case)).values()))
    out['c_bar'] = 4.0 * worst
    fn = os.path.join(GOLD, 'fit_step_cases.npz')
    np.savez_compressed(fn, **out)
    print('%d cases, c = %.3g, %d bytes' % (st.total(), out['c_bar'], os.path.getsize(fn)))
    import json
    mf = os.path.join(GOLD, 'MANIFEST.json')
    man = json.load(open(mf))
    man['fit_step_cases.npz'] = 'inputs of single trust-region steps for sr_expfit_step_probe_f64 (oracle/gen_golden_fit_step.py)'
    with open(mf, 'w') as fp:
        json.dump(man, fp, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
