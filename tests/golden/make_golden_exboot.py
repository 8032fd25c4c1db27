"""tests/golden/exboot.npz: the bootstrap intervals of csrc/xh_exboot_dev.h with every replicate's fit evaluated
to 40 digits (mpmath), and how far the float64 restatement (tests/exboot_np.py) lies from that.

  For the year counts GOLDEN_YEARS of tests/exboot_cases.py and both kinds, on golden_rows(years) (the host rows of
  extremes_cases and six sparse rows), B = 128, confidence 0.90, seed SEED, at T = 2, 10, 100, 1000:  ci_<kind>_<years>
  [rows, 11].  The draws are the restatement's (integer arithmetic: exact), and so are the sorted samples; from a sample on,
  make_golden_extremes.exact_row: exact rational sums, k by root finding at 100 digits, Gamma, exp and log from mpmath, each
  replicate value rounded once to float64; the two order statistics of a bound are picked among those and interpolated in 40
  digits.  Nothing of the product enters.

  np_err_rep_<k|level>_<class> and np_err_ci_<k|level>_<class>: the largest distance of the restatement's replicate values and
  of its bounds from these, in the measures of exboot_cases.rep_errors and ci_errors, per class: ordinary | shifted (the
  series moved by 1e6) | steep (a replicate with t3 > 0.99; a row whose lower bound of k lies below k(t3 = 0.99): k near -1,
  where Gamma(1 + k) magnifies rounding) | flat (a replicate with t3 < -0.99; a row whose upper bound of k lies above
  k(t3 = -0.99) = 7.6).  The tests bound every implementation by 4 x these and not below 4 ulp.

  A replicate that is one value under equal ones has t3 = -1 in exact arithmetic: f(k) = 1 has no root, and the definition's k
  is the tenth Newton iterate on the float64 t3 that every build shares.  So for every flat replicate (float64 t3 < -0.99) k
  is those ten steps on that t3 at 60 digits (newton10), and alpha, xi and the levels follow from it and the exact sums;
  degenerate_replicates counts the ones with t3 = -1 exactly (96).

  python tests/golden/make_golden_exboot.py
"""
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import exboot_cases as xc  # noqa: E402
import exboot_np  # noqa: E402
import extremes_cases as cases  # noqa: E402
import extremes_np  # noqa: E402
import make_golden_extremes as exact  # noqa: E402

mpmath.mp.dps = 40
mpf = mpmath.mpf


FLAT_T3 = [None]                               # the float64 t3 of the replicate at hand when it is flat, else None


def newton10(t3):
    """The definition's k for a float64 t3: Hosking's start and XH_EX_NEWTON = 10 Newton steps, every operation at 60 digits
    (the start's two coefficients are the header's doubles).  Where the steps converge this is the root; for t3 -> -1 it is
    the iterate near 18 that the definition stops at."""
    with mpmath.workdps(60):
        t3 = mpf(float(t3))
        l2, l3 = mpmath.log(2), mpmath.log(3)
        target = (3 + t3) / 2
        c = 2 / (3 + t3) - l2 / l3
        k = mpf(7.8590) * c + (mpf(2.9554) * c) * c
        for _ in range(extremes_np.NEWTON_STEPS):
            A, B = mpmath.expm1(-k * l3), mpmath.expm1(-k * l2)
            f = l3 / l2 if k == 0 else A / B
            if abs(k) < extremes_np.K_DLOG_SERIES:
                dlog = (-(l3 - l2) / 2 + ((l3 * l3 - l2 * l2) / 12) * k) - ((l3 ** 4 - l2 ** 4) / 720) * k ** 3
            else:
                dlog = (l2 * (B + 1)) / B - (l3 * (A + 1)) / A
            k = k - (f - target) / (f * dlog)
        return +k


def k_of_t3(t3, start):
    """For a flat replicate (float64 t3 < -0.99) the ten Newton steps on that t3: its t3 comes within 1e-11 of -1 and reaches
    -1 itself (one low value under equal ones), where f(k) = (3 + t3) / 2 has its root far out or none and the definition's k
    is the tenth iterate.  Elsewhere make_golden_extremes' root, by a bracketing solver."""
    if FLAT_T3[0] is not None:
        return newton10(FLAT_T3[0])
    with mpmath.workdps(100):
        target = (3 + mpf(t3)) / 2
        hi = max(mpf(60), -mpmath.log(target - 1, 2) + 20)
        k = mpmath.findroot(lambda q: exact.f_of_k(q) - target, (mpf(-1), hi), solver='anderson', tol=mpf('1e-75'), maxsteps=2000)
        assert abs(exact.f_of_k(k) - target) < mpf('1e-60')
        return +k


exact.k_of_t3 = k_of_t3                        # (exact_row looks it up in its module)


def exact_fits(starts):
    """replicate_fits of exboot_np in 40 digits; ``starts``: the restatement's values (its t3 says whether a replicate is flat)."""
    at = [0]

    def fits(samples, return_periods):
        assert tuple(return_periods) == cases.GOLDEN_T
        out = np.full((samples.shape[0], exboot_np.NREP + len(return_periods)), np.nan)
        for i, s in enumerate(samples):
            k0, t3f = starts[at[0] + i, 4], starts[at[0] + i, 2]
            FLAT_T3[0] = float(t3f) if (k0 == k0 and t3f < -xc.STEEP_T3) else None
            lows = np.sort(s)
            DEGENERATE[0] += int(lows[0] < lows[1] and lows[1] == lows[-1])
            row, _, fit = exact.exact_row(s, 'max', k0 if k0 == k0 else 0.0, cases.MIN_YEARS)
            assert fit == (k0 == k0), 'the restatement and exact arithmetic disagree on a replicate\'s fit'
            out[i, :2] = row[1:3]
            if fit:
                out[i, 2:] = row[3:6] + row[8:]
        at[0] += samples.shape[0]
        return out
    return fits


DEGENERATE = [0]


def exact_bound(values, p):
    v = sorted(values)
    h = (len(v) - 1) * mpf(p)
    lo = int(mpmath.floor(h))
    hi = min(lo + 1, len(v) - 1)
    return float(mpf(v[lo]) + (mpf(v[hi]) - mpf(v[lo])) * (h - lo))


def main():
    out = {}
    worst = {(w, q, c): 0.0 for w in ('rep', 'ci') for q in xc.QUANTITIES for c in xc.CLASSES}
    k_steep, k_flat = (float(extremes_np.k_of_t3(np.float64(t))) for t in (xc.STEEP_T3, -xc.STEEP_T3))
    p_lo = (1.0 - xc.CONFIDENCE) / 2.0
    p_hi = 1.0 - p_lo
    for ny in xc.GOLDEN_YEARS:
        rows = xc.golden_rows(ny)
        for kind in extremes_np.KINDS:
            table = extremes_np.extremes_rows(rows, kind, (), min_years=cases.MIN_YEARS)[0]
            ci, rep = exboot_np.bootstrap_rows(rows, kind, cases.GOLDEN_T, xc.GOLDEN_B, xc.CONFIDENCE, xc.SEED, min_years=cases.MIN_YEARS)
            # the rows with a fit in the order bootstrap_rows walks them: by n, then by row
            fitted = ~np.isnan(table[:, 5])
            order = [r for n in np.unique(table[fitted, 0]) for r in np.flatnonzero(fitted & (table[:, 0] == n))]
            starts = rep[order].reshape(-1, rep.shape[2])
            _, g_rep = exboot_np.bootstrap_rows(rows, kind, cases.GOLDEN_T, xc.GOLDEN_B, xc.CONFIDENCE, xc.SEED, min_years=cases.MIN_YEARS,
                                                fits=exact_fits(starts))
            assert np.array_equal(np.isnan(rep[:, :, 4:]), np.isnan(g_rep[:, :, 4:])), (ny, kind)
            g_ci = np.full(ci.shape, np.nan)
            g_ci[:, 0] = ci[:, 0]
            for r in np.flatnonzero(~np.isnan(ci[:, 1])):
                fit = ~np.isnan(g_rep[r, :, 4])
                for q in range(1 + len(cases.GOLDEN_T)):
                    lo, hi = (exact_bound(g_rep[r, fit, 4 + q].tolist(), p) for p in (p_lo, p_hi))
                    g_ci[r, 1 + 2 * q], g_ci[r, 2 + 2 * q] = (-hi, -lo) if kind == 'min' and q > 0 else (lo, hi)
            e_rep, e_ci = xc.rep_errors(rep, g_rep), xc.ci_errors(ci, g_ci, table)
            for r in range(rows.shape[0]):
                base = xc.row_class(r, xc.GOLDEN_ROWS)
                for q in xc.QUANTITIES:
                    for b in np.flatnonzero(~np.isnan(e_rep[q][r])):
                        c = base if base == 'shifted' else xc.t3_class(g_rep[r, b, 2])
                        worst[('rep', q, c)] = max(worst[('rep', q, c)], float(e_rep[q][r, b]))
                    if e_ci[q][r] == e_ci[q][r]:
                        c = base if base == 'shifted' else 'steep' if g_ci[r, 1] < k_steep else 'flat' if g_ci[r, 2] > k_flat else 'ordinary'
                        worst[('ci', q, c)] = max(worst[('ci', q, c)], float(e_ci[q][r]))
            out['ci_{}_{}'.format(kind, ny)] = g_ci
            print(ny, kind, 'done', flush=True)
    for (w, q, c), v in worst.items():
        out['np_err_{}_{}_{}'.format(w, q, c)] = np.array(v)
        print('restatement, {:3s} {:6s} {:9s}: {:.3e} = {:.1f} ulp'.format(w, q, c, v, v / cases.EPS))
    out['degenerate_replicates'] = np.array(DEGENERATE[0])
    print('replicates with t3 = -1 exactly:', DEGENERATE[0])
    np.savez_compressed(os.path.join(HERE, 'exboot.npz'), **out)


if __name__ == '__main__':
    main()
