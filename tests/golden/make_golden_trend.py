"""tests/golden/trend.npz: z and p of the Mann-Kendall test to 40 digits (mpmath), rounded once to float64, for the rows of
tests/trend_cases.py (every shape, HOST_ROWS rows each), and how far scipy's double-precision erfc lies from them.

  z = (S -+ 1) / sqrt(V / 18), p = erfc(|z| / sqrt(2)) from the EXACT integers S and V of tests/trend_np.py -- nothing of
  the product and nothing of the reference enters.  scipy_p_relerr is max |erfc_scipy(|z64| 0.70710678118654752) - p| / p
  over the rows with p >= 2.3e-308, z64 the double-precision z of trend_np: the error every float64 evaluation of the
  definition shares (the rounding of z and of the product, magnified by erfc's condition number ~ z^2) plus scipy's own.

  python tests/golden/make_golden_trend.py
"""
import os
import sys

import mpmath
import numpy as np
from scipy import special

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import trend_cases as cases  # noqa: E402
import trend_np  # noqa: E402

mpmath.mp.dps = 40


def main():
    out = {}
    worst = 0.0
    for ns, ny in cases.SHAPES:
        rows = cases.make_rows(ns, ny, cases.HOST_ROWS)
        z = np.full(len(rows), np.nan)
        p = np.full(len(rows), np.nan)
        for r, x in enumerate(rows):
            n, S, V, slopes = trend_np.trend_counts(x, ns)
            if n < 4 or slopes.size == 0:
                continue
            zz = mpmath.mpf(0)
            if V != 0 and S != 0:
                zz = (mpmath.mpf(S) - (1 if S > 0 else -1)) / mpmath.sqrt(mpmath.mpf(V) / 18)
            pp = mpmath.erfc(abs(zz) / mpmath.sqrt(2))
            z[r], p[r] = float(zz), float(pp)
            z64 = trend_np.trend_row(x, ns, cases.Z95)[3]
            if pp >= cases.TINY:
                err = abs(mpmath.mpf(float(special.erfc(abs(z64) * 0.70710678118654752))) - pp) / pp
                worst = max(worst, float(err))
        out['z_{}_{}'.format(ns, ny)] = z
        out['p_{}_{}'.format(ns, ny)] = p
    out['scipy_p_relerr'] = np.array(worst)
    np.savez_compressed(os.path.join(HERE, 'trend.npz'), **out)
    print('scipy erfc max relative error of p: {:.3e} = {:.1f} ulp'.format(worst, worst / np.finfo(float).eps))


if __name__ == '__main__':
    main()
