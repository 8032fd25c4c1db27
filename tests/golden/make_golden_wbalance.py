"""40-digit values of every column of xh_water_balance on the rows of tests/wbalance_cases.py -> tests/golden/wbalance.npz.

    python tests/golden/make_golden_wbalance.py

The values are the definition's in exact arithmetic on the doubles of the rows (mpmath, 40 digits): sums are exact
sums, the medians use the exact e_y, Fu's curve is the definition's own form with mpmath's log, exp, log1p and expm1, and omega is
the root of the definition's equation found by 160 bisection steps on s = log(omega - 1) at 50 digits.  Every batch twice, with
its AET (`*_<years>`) and without (`*_noaet_<years>`).  Stored as a rounded double and the remainder (`*_lo`), so that a test
forms value - golden to far below an ulp.  The script also measures how far the numpy restatement (tests/wbalance_np.py) lies from
them, per quantity, over all rows and year counts:
    dist_table [21], dist_annual, dist_xcorr   the largest |restatement - golden| / |golden| (absolute where golden = 0)
with two columns in the measures the tests bound them by:
    omega        |restatement - golden| / golden
    budyko_dev   |restatement - golden| / max(|golden|, 1)
`undef_*` [rows, 21] marks the quotients whose exact denominator is 0, which have no value and enter no distance.  It prints the
distances; tests/test_wbalance_host.py quotes them."""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import wbalance_cases as cases  # noqa: E402
import wbalance_np as wnp  # noqa: E402

mp.mp.dps = 50
NAN = mp.mpf('nan')
S_LO, S_HI = mp.mpf(wnp.S_LO), mp.mpf(wnp.S_HI)


def excess(m, lr, omega):
    return m * mp.expm1(mp.log1p(mp.exp(omega * lr)) / omega)


def fu(phi, omega):
    lo, m = min(mp.mpf(1), phi), max(mp.mpf(1), phi)
    if lo == 0:
        return mp.mpf(0)
    return lo - excess(m, mp.log(lo / m), omega)


def omega_of(phi, eps):
    lo, m = min(mp.mpf(1), phi), max(mp.mpf(1), phi)
    if not (0 < eps < lo):
        return NAN
    lr, target = mp.log(lo / m), lo - eps
    a, b = S_LO, S_HI
    if not (excess(m, lr, 1 + mp.exp(b)) < target < excess(m, lr, 1 + mp.exp(a))):
        return NAN
    for _ in range(160):
        mid = (a + b) / 2
        if excess(m, lr, 1 + mp.exp(mid)) > target:
            a = mid
        else:
            b = mid
    return 1 + mp.exp((a + b) / 2)


def median(values):
    a = sorted(values)
    n = len(a)
    return (a[(n - 1) // 2] + a[n // 2]) / 2


def div(n, d):
    """(n / d, undefined): IEEE's answer where d = 0 has no 40-digit value."""
    return (NAN, True) if d == 0 else (n / d, False)


def golden_row(p, pet, q, aet, max_lag, omega0):
    ncol = p.size
    nyear = ncol // 12
    given = [p, pet, q] + ([aet] if aet is not None else [])
    inc = np.logical_and.reduce([np.isfinite(v) for v in given])
    P, E, Q = ([mp.mpf(float(e) + 0.0) if k else None for e, k in zip(v, inc)] for v in (p, pet, q))
    A = [mp.mpf(float(e) + 0.0) if k else None for e, k in zip(aet, inc)] if aet is not None else None
    table, undef = [NAN] * wnp.NCOL, [False] * wnp.NCOL
    annual = [[NAN] * nyear for _ in range(4)]
    xcorr = [NAN] * (max_lag + 1)
    months = [t for t in range(ncol) if inc[t]]
    nm = len(months)
    table[1] = mp.mpf(nm)
    whole = [y for y in range(nyear) if inc[12 * y:12 * y + 12].all()]
    ny = len(whole)
    table[0] = mp.mpf(ny)
    if nm:
        table[18] = mp.mpf(sum(1 for t in months if P[t] < E[t])) / nm
        mP, mQ = mp.fsum(P[t] for t in months) / nm, mp.fsum(Q[t] for t in months) / nm
        den = mp.sqrt(mp.fsum((P[t] - mP) ** 2 for t in months) * mp.fsum((Q[t] - mQ) ** 2 for t in months))
        for k in range(max_lag + 1):
            num = mp.fsum((P[t] - mP) * (Q[t + k] - mQ) for t in months if t + k < ncol and inc[t + k])
            xcorr[k] = num / den if den != 0 else NAN
        numbers = [k for k in range(max_lag + 1) if not mp.isnan(xcorr[k])]
        if numbers:
            best = max(numbers, key=lambda k: (xcorr[k], -k))
            table[19], table[20] = mp.mpf(best), xcorr[best]
        undef[19] = undef[20] = den == 0
    if ny == 0:
        return table, annual, xcorr, undef
    for v, x in enumerate((P, E, A, Q)):
        if x is not None:
            for y in whole:
                annual[v][y] = mp.fsum(x[12 * y:12 * y + 12])
    pbar, petbar, qbar = (mp.fsum(annual[v][y] for y in whole) / ny for v in (0, 1, 3))
    aetbar = mp.fsum(annual[2][y] for y in whole) / ny if A is not None else NAN
    table[2], table[3], table[4], table[5] = pbar, petbar, aetbar, qbar
    residual = (pbar - aetbar) - qbar
    table[9] = residual
    for col, num in ((6, qbar), (7, petbar), (8, aetbar), (10, residual)):
        table[col], undef[col] = div(num, pbar)
    if pbar != 0:
        phi, eps = petbar / pbar, (pbar - qbar) / pbar
        table[11], table[12] = omega_of(phi, eps), eps - fu(phi, mp.mpf(omega0))
    else:
        undef[11] = undef[12] = True
    dp, de, dq = ({y: annual[v][y] - bar for y in whole} for v, bar in ((0, pbar), (1, petbar), (3, qbar)))
    if qbar > 0:
        for col, d, bar in ((13, dp, pbar), (14, de, petbar)):
            e = [(dq[y] / d[y]) * (bar / qbar) for y in whole if d[y] != 0]
            if e:
                table[col] = median(e)
    if pbar != 0 and petbar != 0 and qbar != 0:
        x1, x2, z = ({y: d[y] / bar for y in whole} for d, bar in ((dp, pbar), (de, petbar), (dq, qbar)))
        s11, s12, s22, s1z, s2z = (mp.fsum(a[y] * b[y] for y in whole) for a, b in ((x1, x1), (x1, x2), (x2, x2), (x1, z), (x2, z)))
        det = s11 * s22 - s12 * s12
        if ny >= 3 and det > 0:
            table[15], table[16] = (s1z * s22 - s2z * s12) / det, (s2z * s11 - s1z * s12) / det
    else:
        undef[15] = undef[16] = True
    spq, spp, sqq = (mp.fsum(a[y] * b[y] for y in whole) for a, b in ((dp, dq), (dp, dp), (dq, dq)))
    if spp * sqq > 0:
        table[17] = spq / mp.sqrt(spp * sqq)
    return table, annual, xcorr, undef


def split(values):
    """mpf values -> (rounded doubles, remainders)."""
    hi = np.array([float(e) for e in values], dtype=np.float64)
    lo = np.array([float(e - mp.mpf(h)) if mp.isfinite(e) and np.isfinite(h) else 0.0 for e, h in zip(values, hi)], dtype=np.float64)
    return hi, lo


def rel(got, want):
    """|got - want| / |want| per element (absolute where want = 0); 0 where both are NaN; inf where one is."""
    out = []
    for g, w in zip(got, want):
        if mp.isnan(w) or np.isnan(g):
            out.append(0.0 if (mp.isnan(w) and np.isnan(g)) else np.inf)
        else:
            d = abs(mp.mpf(float(g)) - w)
            out.append(float(d / abs(w)) if w != 0 else float(d))
    return np.array(out)


def main():
    out = {'years': np.array(cases.YEARS), 'max_lag': np.array(cases.MAX_LAG), 'omega0': np.array(cases.OMEGA0)}
    dist_table = np.zeros(wnp.NCOL)
    dist_annual = dist_xcorr = 0.0
    for ny in cases.YEARS:
        p, pet, q, aet = cases.rows(ny)
        for tag, a in (('', aet), ('_noaet', None)):
            r_table, r_annual, r_xcorr = wnp.water_balance(p, pet, q, a, 0, ny, cases.MAX_LAG, cases.OMEGA0)
            g = [golden_row(p[i], pet[i], q[i], None if a is None else a[i], cases.MAX_LAG, cases.OMEGA0) for i in range(p.shape[0])]
            for name, k, shape in (('table', 0, (wnp.NCOL,)), ('xcorr', 2, (cases.MAX_LAG + 1,))):        # (the annual totals are sums of
                hi, lo = zip(*(split(e[k]) for e in g))                                                 # 12: measured, not stored)
                out['{}{}_{}'.format(name, tag, ny)] = np.array(hi).reshape((len(g),) + shape)
                out['{}_lo{}_{}'.format(name, tag, ny)] = np.array(lo).reshape((len(g),) + shape)
            out['undef{}_{}'.format(tag, ny)] = np.array([e[3] for e in g], dtype=bool)
            for i, (t, ann, xc, undef) in enumerate(g):
                d = np.where(undef, 0.0, rel(r_table[i], t))
                if not mp.isnan(t[12]):
                    d[12] = float(abs(mp.mpf(float(r_table[i, 12])) - t[12]) / max(abs(t[12]), 1))
                assert np.isfinite(d).all(), (ny, tag, cases.KINDS[i], [wnp.COLUMNS[c] for c in np.nonzero(~np.isfinite(d))[0]])
                dist_table = np.maximum(dist_table, d)
                dist_annual = max(dist_annual, float(rel(r_annual[i].ravel(), sum(ann, [])).max()))
                if not undef[20]:
                    dist_xcorr = max(dist_xcorr, float(rel(r_xcorr[i], xc).max()))
    out['dist_table'], out['dist_annual'], out['dist_xcorr'] = dist_table, np.array(dist_annual), np.array(dist_xcorr)
    np.savez_compressed(os.path.join(HERE, 'wbalance.npz'), **out)
    for name, d in zip(wnp.COLUMNS, dist_table):
        print('{:14s} {:.3e}'.format(name, d))
    print('{:14s} {:.3e}\n{:14s} {:.3e}'.format('annual', dist_annual, 'xcorr', dist_xcorr))


if __name__ == '__main__':
    main()
