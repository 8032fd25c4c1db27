"""40-digit values of every column of xh_signatures on the rows of tests/signatures_cases.py -> tests/golden/signatures.npz.

    python tests/golden/make_golden_signatures.py

The values are the definition's in exact arithmetic on the doubles of the rows (mpmath, 40 digits): sums are
exact sums, the order statistics use the exact h = (n - 1) p of the double p, log and atan2 are mpmath's.  Stored per year count
as a rounded double and the remainder (`*_lo`), so that a test forms value - golden to far below an ulp.  The script also
measures how far the numpy restatement (tests/signatures_np.py) lies from them, per quantity, over all rows and year counts:
    dist_table [18], dist_fdc, dist_regime   the largest |restatement - golden| / |golden| (absolute where golden = 0)
with two columns in the measures the tests bound them by:
    fdc_slope   |restatement - golden| / max(|golden|, 1)
    centroid    the circular distance in months times the row's concentration (the relative error of the vector (C, S): the
                angle of a vector whose length goes to 0 is undefined)
`undef_<years>` [rows, 18] marks the quotients whose exact denominator is 0 (lag1 of a constant row: 0 / 0), which have no value
and enter no distance.  It prints the distances; tests/test_signatures_host.py quotes them."""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import signatures_cases as cases  # noqa: E402
import signatures_np as snp  # noqa: E402

mp.mp.dps = 40
NAN = mp.mpf('nan')


def quantile(a, p):
    n = len(a)
    h = (n - 1) * mp.mpf(float(p))
    lo = int(mp.floor(h))
    hi = min(lo + 1, n - 1)
    return a[lo] + (a[hi] - a[lo]) * (h - lo)


def golden_row(x, cal0, probs):
    ncol = x.size
    nyear = ncol // 12
    keep = np.isfinite(x)
    v = [mp.mpf(float(e) + 0.0) if k else None for e, k in zip(x, keep)]
    table = [NAN] * snp.NCOL
    undef = [False] * snp.NCOL                      # a quotient whose exact denominator is 0: no value to hold anything to
    fdc = [NAN] * len(probs)
    regime = [NAN] * 12
    inc = [e for e in v if e is not None]
    n = len(inc)
    whole = [y for y in range(nyear) if all(keep[12 * y:12 * y + 12])]
    table[0], table[1], table[15] = mp.mpf(n), mp.mpf(sum(1 for e in inc if e == 0)), mp.mpf(len(whole))
    count = [0] * 12
    for m in range(12):
        sel = [v[t] for t in range((m - cal0 + 12) % 12, ncol, 12) if v[t] is not None]
        count[m] = len(sel)
        if sel:
            regime[m] = mp.fsum(sel) / len(sel)
    if n == 0:
        return table, fdc, regime, undef
    a = sorted(inc)
    fdc = [quantile(a, p) for p in probs]
    sx = mp.fsum(inc)
    mean = sx / n
    sxx = mp.fsum((e - mean) ** 2 for e in inc)
    pairs = [(v[t], v[t + 1]) for t in range(ncol - 1) if v[t] is not None and v[t + 1] is not None]
    table[2] = mean
    if n >= 2:
        table[3] = mp.sqrt(sxx / (n - 1))
        table[4] = table[3] / mean if mean != 0 else NAN
        table[6] = mp.fsum((p - mean) * (q - mean) for p, q in pairs) / sxx if sxx != 0 else NAN
        undef[4], undef[6] = mean == 0, sxx == 0
    table[5] = quantile(a, 0.5)
    table[7] = mp.fsum(abs(q - p) for p, q in pairs) / sx if sx != 0 else NAN
    undef[7] = sx == 0
    q67, q34 = quantile(a, 0.67), quantile(a, 0.34)
    if q34 > 0:
        table[8] = (mp.log(q67) - mp.log(q34)) / mp.mpf(0.33)
    if all(c > 0 for c in count):
        R = mp.fsum(regime)
        C = mp.fsum(regime[m] * mp.mpf(float(snp.COS[m])) for m in range(12))
        S = mp.fsum(regime[m] * mp.mpf(float(snp.SIN[m])) for m in range(12))
        table[9] = R
        table[10] = mp.mpf(1 + max(range(12), key=lambda m: (regime[m], -m)))
        table[11] = mp.mpf(1 + min(range(12), key=lambda m: (regime[m], m)))
        undef[12] = undef[14] = R == 0
        if R != 0:
            table[12] = mp.fsum(abs(regime[m] - R / 12) for m in range(12)) / R
            table[14] = mp.sqrt(C * C + S * S) / R
        cen = mp.atan2(S, C) * mp.mpf(snp.MONTHS_PER_RADIAN)
        table[13] = cen + 12 if cen < 0 else cen
    if whole:
        A = [mp.fsum(v[12 * y:12 * y + 12]) for y in whole]
        amean = mp.fsum(A) / len(A)
        table[16] = amean
        undef[17] = len(A) >= 2 and amean == 0
        if len(A) >= 2 and amean != 0:
            table[17] = mp.sqrt(mp.fsum((e - amean) ** 2 for e in A) / (len(A) - 1)) / amean
    return table, fdc, regime, undef


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
    probs = snp.probabilities(cases.EXCEEDANCE)
    out = {'years': np.array(cases.YEARS), 'cal0': np.array(cases.CAL0), 'exceedance': np.array(cases.EXCEEDANCE, dtype=np.float64)}
    dist_table = np.zeros(snp.NCOL)
    dist_fdc = dist_regime = 0.0
    for ny in cases.YEARS:
        x = cases.rows(ny)
        r_table, r_fdc, r_regime = snp.signatures(x, 0, ny, cases.CAL0, probs)
        g = [golden_row(row, cases.CAL0, probs) for row in x]
        for name, k, width in (('table', 0, snp.NCOL), ('fdc', 1, len(probs)), ('regime', 2, 12)):
            hi, lo = zip(*(split(e[k]) for e in g))
            out['{}_{}'.format(name, ny)] = np.array(hi).reshape(len(g), width)
            out['{}_lo_{}'.format(name, ny)] = np.array(lo).reshape(len(g), width)
        out['undef_{}'.format(ny)] = np.array([e[3] for e in g], dtype=bool)
        for i, (t, f, m, undef) in enumerate(g):
            d = np.where(undef, 0.0, rel(r_table[i], t))
            if not mp.isnan(t[8]):
                d[8] = float(abs(mp.mpf(float(r_table[i, 8])) - t[8]) / max(abs(t[8]), 1))
            if not mp.isnan(t[13]):
                c = abs(mp.mpf(float(r_table[i, 13])) - t[13])
                conc = t[14] if not mp.isnan(t[14]) else mp.mpf(1)
                d[13] = float(min(c, 12 - c) * conc)
            dist_table = np.maximum(dist_table, d)
            dist_fdc = max(dist_fdc, float(rel(r_fdc[i], f).max()))
            dist_regime = max(dist_regime, float(rel(r_regime[i], m).max()))
    out['dist_table'], out['dist_fdc'], out['dist_regime'] = dist_table, np.array(dist_fdc), np.array(dist_regime)
    np.savez_compressed(os.path.join(HERE, 'signatures.npz'), **out)
    for name, d in zip(snp.COLUMNS, dist_table):
        print('{:14s} {:.3e}'.format(name, d))
    print('{:14s} {:.3e}\n{:14s} {:.3e}'.format('fdc', dist_fdc, 'regime', dist_regime))


if __name__ == '__main__':
    main()
