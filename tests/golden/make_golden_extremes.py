"""tests/golden/extremes.npz: the extreme-value definition of csrc/xh_extremes_dev.h evaluated to 40 digits (mpmath), rounded
once to float64, and how far the float64 restatement (tests/extremes_np.py) lies from it.

  For every year count of tests/extremes_cases.py and both kinds, on the first HOST_ROWS rows: table_<kind>_<years> [rows, 12] =
  n, l1, l2, t3, t4, k, alpha, xi and the return levels at T = 2, 10, 100, 1000, and T_year_<kind>_<years> [rows, years].  The
  annual series is the restatement's (comparisons only: exact); from it on everything is exact rational arithmetic on the
  doubles and 40-digit functions -- the L-moments as sum_i C(i, r) / C(n - 1, r) z_(i) / n, k by root finding on
  (1 - 3^-k) / (1 - 2^-k) = (3 + t3) / 2 at 100 digits, Gamma, exp and log from mpmath.  Nothing of the product enters.

  sweep_t3 [m] and sweep_k, sweep_alpha (alpha / l2), sweep_xi ((xi - l1) / l2) [m]: the pieces over t3 values that put k at 0
  (to the rounding of t3), +-1e-12, +-1e-8, +-1e-5, +-1e-3, on both sides of +-2^-7 and +-0.25 (the header's two switch-overs),
  and t3 from -0.95 to 0.95 and on to 0.99.

  np_err_<quantity>_<class>: the largest error of the restatement in the measure of extremes_cases.errors over the rows with a
  fit, measured on MEASURED_ROWS = 300 rows a year count and kind (the rows of the GPU test, of which the first HOST_ROWS are
  stored), per row class (ordinary | shifted: the series moved by 1e6, whose 2 b1 - b0 cancels);  np_err_sweep_<k|alpha|xi>:
  the same for the pieces over the sweep.  The tests bound every implementation by 4 x these.  lmom is the error of l1, l2, t3
  and t4 (extremes_cases.lmom_error);  scipy_err_lmom_<class>: that of scipy.stats.lmoment(order = 1 .. 4, standardize) on the
  same annual series, so that the restatement and scipy, two summations, are compared within the sum of their own errors.

  python tests/golden/make_golden_extremes.py
"""
import os
import sys

import mpmath
import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import extremes_cases as cases  # noqa: E402
import extremes_np  # noqa: E402

mpmath.mp.dps = 40
mpf = mpmath.mpf
MEASURED_ROWS = 300
T3_MAX = mpf(1) - mpf(2) ** -20


def f_of_k(k):
    return mpmath.log(3) / mpmath.log(2) if k == 0 else (1 - mpf(3) ** -k) / (1 - mpf(2) ** -k)


def t3_of_k(k):
    return 2 * f_of_k(mpf(k)) - 3


def k_of_t3(t3, start):
    with mpmath.workdps(100):
        target = (3 + mpf(t3)) / 2
        k = mpmath.findroot(lambda q: f_of_k(q) - target, (mpf(start) - mpf('1e-3'), mpf(start) + mpf('1e-3')), solver='secant',
                            tol=mpf('1e-75'), maxsteps=200)
        assert abs(f_of_k(k) - target) < mpf('1e-60')
        return +k


def pieces(k):
    """alpha / l2 and (xi - l1) / l2."""
    gam = mpmath.gamma(1 + k)
    if k == 0:
        a = 1 / mpmath.log(2)
        return a, -mpmath.euler * a
    a = k / ((1 - mpf(2) ** -k) * gam)
    return a, -a * (1 - gam) / k


def quantile(T, k, alpha, xi):
    y = -mpmath.log1p(-1 / mpf(T))
    return xi - alpha * mpmath.log(y) if k == 0 else xi - alpha * mpmath.expm1(k * mpmath.log(y)) / k


def return_period(z, k, alpha, xi):
    s = (mpf(z) - xi) / alpha
    if k == 0:
        u = mpmath.exp(-s)
    elif 1 - k * s <= 0:
        return mpf(1) if k < 0 else mpmath.inf
    else:
        u = (1 - k * s) ** (1 / k)
    return -1 / mpmath.expm1(-u)


def exact_row(a, kind, start_k, min_years):
    """The 12 table columns and T_y of one annual series, or the columns of a row without a fit."""
    sign = -1 if kind == 'min' else 1
    z = sorted(sign * float(v) for v in a if v == v)
    n = len(z)
    out = [float(n)] + [np.nan] * 11
    T_year = np.full(a.size, np.nan)
    b = []
    for r in range(min(4, n)):
        tot = mpf(0)
        for i, v in enumerate(z):
            w = mpf(1)
            for j in range(1, r + 1):
                w = w * (i - j + 1) / (n - j)
            tot += w * mpf(v)
        b.append(tot / n)
    if n >= 1:
        out[1] = float(sign * b[0])
    if n >= 2:
        out[2] = float(2 * b[1] - b[0])
    if n < min_years or n < 4 or z[0] == z[-1]:
        return out, T_year, False
    l1, l2 = b[0], 2 * b[1] - b[0]
    if not l2 > 0:
        return out, T_year, False
    t3, t4 = (6 * b[2] - 6 * b[1] + b[0]) / l2, (20 * b[3] - 30 * b[2] + 12 * b[1] - b[0]) / l2
    if t3 > T3_MAX:
        return out, T_year, False
    k = k_of_t3(t3, start_k)
    ra, rx = pieces(k)
    alpha, xi = ra * l2, l1 + rx * l2
    out[3:8] = [float(t3), float(t4), float(k), float(alpha), float(sign * xi)]
    out[8:] = [float(sign * quantile(T, k, alpha, xi)) for T in cases.GOLDEN_T]
    for y, v in enumerate(a):
        if v == v:
            T_year[y] = float(return_period(sign * float(v), k, alpha, xi))
    return out, T_year, True


def sweep_t3():
    ks = [0.0]
    for m in (1e-12, 1e-8, 1e-5, 1e-3, 0.0078125 * (1 - 1e-3), 0.0078125 * (1 + 1e-3), 0.25 * (1 - 1e-6), 0.25 * (1 + 1e-6)):
        ks += [m, -m]
    t3 = [float(t3_of_k(k)) for k in ks]
    t3 += list(np.linspace(-0.95, 0.95, 39)) + [-0.949, 0.949, 0.97, 0.99]
    return np.array(t3)


def main():
    out = {}
    worst = {(q, c): 0.0 for q in cases.QUANTITIES for c in cases.CLASSES}
    scipy_worst = {c: 0.0 for c in cases.CLASSES}
    for ny in cases.YEARS:
        rows = cases.make_rows(ny, MEASURED_ROWS)
        for kind in extremes_np.KINDS:
            table, annual, T_year = extremes_np.extremes_rows(rows, kind, cases.GOLDEN_T, min_years=cases.MIN_YEARS)
            g_table = np.full(table.shape, np.nan)
            g_T = np.full(T_year.shape, np.nan)
            for r in range(MEASURED_ROWS):
                start = table[r, 5] if table[r, 5] == table[r, 5] else 0.0
                g_table[r], g_T[r], fit = exact_row(annual[r], kind, start, cases.MIN_YEARS)
                assert fit == (table[r, 5] == table[r, 5]), (ny, kind, r, 'the restatement and exact arithmetic disagree on the fit')
            assert cases.same_masks(table, annual, T_year, g_table, annual, g_T), (ny, kind)
            err = cases.errors(table, T_year, g_table, g_T)
            for q in cases.QUANTITIES:
                for r in range(MEASURED_ROWS):
                    if err[q][r] == err[q][r]:
                        key = (q, cases.class_of(r))
                        worst[key] = max(worst[key], float(err[q][r]))
            # scipy's own sample L-moments (another summation) on the same annual series, against the same values
            sign = -1.0 if kind == 'min' else 1.0
            for r in range(MEASURED_ROWS):
                if g_table[r, 5] == g_table[r, 5]:
                    z = sign * annual[r][~np.isnan(annual[r])]
                    lm = np.array(stats.lmoment(z, order=[1, 2, 3, 4], standardize=True), dtype=np.float64)
                    ref = g_table[r, 1:5] * [sign, 1.0, 1.0, 1.0]
                    e = float(cases.lmom_error(lm[None, :], ref[None, :])[0])
                    scipy_worst[cases.class_of(r)] = max(scipy_worst[cases.class_of(r)], e)
            out['table_{}_{}'.format(kind, ny)] = g_table[:cases.HOST_ROWS]
            out['T_year_{}_{}'.format(kind, ny)] = g_T[:cases.HOST_ROWS]
            print(ny, kind, 'done', flush=True)
    for (q, c), v in worst.items():
        out['np_err_{}_{}'.format(q, c)] = np.array(v)
        print('restatement, {:8s} {:9s}: {:.3e} = {:.1f} ulp'.format(q, c, v, v / cases.EPS))
    for c, v in scipy_worst.items():
        out['scipy_err_lmom_' + c] = np.array(v)
        print('scipy.stats.lmoment, {:9s}: {:.3e} = {:.1f} ulp'.format(c, v, v / cases.EPS))
    t3 = sweep_t3()
    start = extremes_np.k_of_t3(t3)
    gk = [k_of_t3(t, s) for t, s in zip(t3, start)]
    ga, gx = zip(*[pieces(k) for k in gk])
    out['sweep_t3'] = t3
    out['sweep_k'], out['sweep_alpha'], out['sweep_xi'] = (np.array([float(v) for v in col]) for col in (gk, ga, gx))
    one, zero = np.ones(t3.size), np.zeros(t3.size)
    alpha, xi = extremes_np.gev_parameters(zero, one, start)
    err = cases.sweep_errors(start, alpha, xi, out['sweep_k'], out['sweep_alpha'], out['sweep_xi'])
    for name in ('k', 'alpha', 'xi'):
        e = float(err[name].max())
        out['np_err_sweep_' + name] = np.array(e)
        print('restatement, sweep {:6s}: {:.3e} = {:.1f} ulp'.format(name, e, e / cases.EPS))
    np.savez_compressed(os.path.join(HERE, 'extremes.npz'), **out)


if __name__ == '__main__':
    main()
