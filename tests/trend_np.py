"""The trend statistics of xh_trend (include/xanthos_hip.h, csrc/xh_trend_dev.h) in plain numpy: every pairwise slope is
formed and stored, np.sort orders them, np.median takes the medians.  The yardstick of the trend tests: the product selects
the same order statistics without storing a slope."""
import math

import numpy as np

COLUMNS = ('n', 's', 'var_s', 'z', 'p', 'slope', 'intercept', 'slope_lo', 'slope_hi', 'npairs')


def trend_counts(x, nseason):
    """(n, S, V, slopes) of one row: exact integers and every pairwise slope, unsorted."""
    x = np.asarray(x, dtype=np.float64)
    ncol = x.size
    assert ncol > 0 and ncol % nseason == 0
    fin = np.isfinite(x)
    t = np.arange(ncol)
    S = V = 0
    slopes = []
    for m in range(nseason):
        idx = t[m::nseason][fin[m::nseason]]
        xm = x[idx]
        nm = xm.size
        V += nm * (nm - 1) * (2 * nm + 5)
        # sum over the elements of (e - 1)(2 e + 5) = sum over the tie groups of g (g - 1)(2 g + 5)
        g = np.unique(xm, return_counts=True)[1].astype(np.int64)
        V -= int((g * (g - 1) * (2 * g + 5)).sum())
        i, j = np.triu_indices(nm, 1)
        S += int((xm[j] > xm[i]).sum()) - int((xm[j] < xm[i]).sum())
        with np.errstate(invalid='ignore', over='ignore'):
            slopes.append((xm[j] - xm[i]) / ((idx[j] - idx[i]) // nseason).astype(np.float64))
    return int(fin.sum()), S, V, (np.concatenate(slopes) if slopes else np.zeros(0))


def trend_row(x, nseason, z_conf):
    """The ten columns of one row (the used window)."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    tau = np.arange(x.size).astype(np.float64) / np.float64(nseason)
    n, S, V, slopes = trend_counts(x, nseason)
    N = slopes.size
    out = np.full(10, np.nan)
    out[0], out[9] = n, N
    if n < 4 or N == 0:
        return out
    slopes = slopes + 0.0                      # -0.0 counts as +0.0
    var_s = float(V) / 18.0
    sigma = math.sqrt(var_s)
    z = 0.0
    if var_s != 0.0 and S > 0:
        z = (S - 1) / sigma
    elif var_s != 0.0 and S < 0:
        z = (S + 1) / sigma
    p = math.erfc(abs(z) * 0.70710678118654752)
    srt = np.sort(slopes)
    slope = np.median(slopes)
    ru = min(int(np.round((N - z_conf * sigma) / 2.0)), N - 1)
    rl = max(int(np.round((N + z_conf * sigma) / 2.0)) - 1, 0)
    intercept = np.median(x[fin]) - slope * np.median(tau[fin])
    out[1:9] = S, var_s, z, p, slope, intercept, srt[rl], srt[ru]
    return out


def trend_rows(rows, nseason, z_conf, start=0, ncol=None):
    rows = np.asarray(rows, dtype=np.float64)
    ncol = rows.shape[1] - start if ncol is None else ncol
    return np.array([trend_row(r[start:start + ncol], nseason, z_conf) for r in rows]).reshape(-1, 10)
