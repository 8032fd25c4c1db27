"""numpy restatement of xh_signatures (include/xanthos_hip.h, csrc/xh_signatures_dev.h), row by row: the 256
strided partial sums joined by the tree of xh_block_sum256 for the S256 sums, np.cumsum (sequential) for the sequential sums,
np.sort for the order statistics and the linear rule written out.  Every column is what the definition's operations give in
IEEE double; only log (fdc_slope) and atan2 (centroid) come from numpy's library instead of the compiler's."""
import numpy as np

COLUMNS = ('n', 'n_zero', 'mean', 'std', 'cv', 'median', 'lag1', 'flashiness', 'fdc_slope', 'regime_total', 'peak_month',
           'low_month', 'seasonality', 'centroid', 'concentration', 'n_years', 'annual_mean', 'annual_cv')
NCOL = len(COLUMNS)
EXCEEDANCE = (1, 5, 10, 20, 50, 80, 90, 95, 99)
MONTHS_PER_RADIAN = 1.909859317102744          # 6 / pi, correctly rounded
COS = np.array([0.9659258262890683, 0.7071067811865476, 0.25881904510252074, -0.25881904510252074, -0.7071067811865476,
                -0.9659258262890683, -0.9659258262890683, -0.7071067811865476, -0.25881904510252074, 0.25881904510252074,
                0.7071067811865476, 0.9659258262890683])
SIN = np.array([0.25881904510252074, 0.7071067811865476, 0.9659258262890683, 0.9659258262890683, 0.7071067811865476,
                0.25881904510252074, -0.25881904510252074, -0.7071067811865476, -0.9659258262890683, -0.9659258262890683,
                -0.7071067811865476, -0.25881904510252074])


def probabilities(exceedance=EXCEEDANCE):
    """The non-exceedance probabilities of the exceedance percents."""
    return np.array([(100.0 - float(p)) / 100.0 for p in exceedance], dtype=np.float64)


def seq_sum(v):
    """From 0.0 in ascending index order."""
    v = np.asarray(v, dtype=np.float64)
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def s256(terms, keep):
    """S256 of terms[t] over the t with keep[t]: a term left out adds nothing (0.0 added to a partial sum that started at +0.0
    leaves its bits)."""
    f = np.where(keep, terms, 0.0)
    pad = (-f.size) % 256
    f = np.concatenate([f, np.zeros(pad)]).reshape(-1, 256)
    part = np.zeros(256)
    for row in f:
        part = part + row
    stride = 128
    while stride > 0:
        part[:stride] = part[:stride] + part[stride:2 * stride]
        stride //= 2
    return float(part[0])


def quantile(a, p):
    """numpy's `linear` rule on the sorted a."""
    n = a.size
    h = np.float64(n - 1) * np.float64(p)
    fl = np.floor(h)
    g = h - fl
    lo = int(fl)
    hi = min(lo + 1, n - 1)
    d = a[hi] - a[lo]
    return float(a[lo] + d * g) if g < 0.5 else float(a[hi] - d * (1.0 - g))


def signature_row(x, cal0=0, probs=()):
    """(table [18], fdc [nP], regime [12]) of one window x [12 nyear]."""
    with np.errstate(all='ignore'):
        x = np.asarray(x, dtype=np.float64) + 0.0
        ncol = x.size
        nyear = ncol // 12
        assert ncol == 12 * nyear and nyear >= 1
        keep = np.isfinite(x)
        xz = np.where(keep, x, 0.0)
        table = np.full(NCOL, np.nan)
        fdc = np.full(len(probs), np.nan)
        regime = np.full(12, np.nan)
        n = int(keep.sum())
        years = x.reshape(nyear, 12)
        whole = np.isfinite(years).all(axis=1)
        table[0], table[1], table[15] = n, int((keep & (x == 0.0)).sum()), int(whole.sum())
        # the calendar means
        count = np.zeros(12)
        for m in range(12):
            sel = np.arange((m - cal0 + 12) % 12, ncol, 12)
            v = x[sel][keep[sel]]
            count[m] = v.size
            if v.size:
                regime[m] = np.float64(seq_sum(v)) / np.float64(v.size)
        if n == 0:
            return table, fdc, regime
        a = np.sort(x[keep])
        for j, p in enumerate(probs):
            fdc[j] = quantile(a, p)
        sx = s256(xz, keep)
        mean = np.float64(sx) / np.float64(n)
        dev = xz - mean
        sxx = s256(dev * dev, keep)
        pair = keep[:-1] & keep[1:]
        sprod = s256(dev[:-1] * dev[1:], pair)
        sabs = s256(np.abs(xz[1:] - xz[:-1]), pair)
        sd = np.sqrt(np.float64(sxx) / np.float64(n - 1)) if n >= 2 else np.nan
        table[2], table[3], table[4], table[5] = mean, sd, sd / mean, quantile(a, 0.5)
        table[6] = np.float64(sprod) / np.float64(sxx) if n >= 2 else np.nan
        table[7] = np.float64(sabs) / np.float64(sx)
        q67, q34 = quantile(a, 0.67), quantile(a, 0.34)
        table[8] = (np.log(q67) - np.log(q34)) / 0.33 if q34 > 0.0 else np.nan
        if (count > 0).all():
            R = np.float64(seq_sum(regime))
            C = np.float64(seq_sum(regime * COS))
            S = np.float64(seq_sum(regime * SIN))
            centroid = np.arctan2(S, C) * MONTHS_PER_RADIAN
            if centroid < 0.0:
                centroid = centroid + 12.0
            table[9], table[10], table[11] = R, 1 + int(np.argmax(regime)), 1 + int(np.argmin(regime))
            table[12] = np.float64(seq_sum(np.abs(regime - R / 12.0))) / R
            table[13], table[14] = centroid, np.sqrt(C * C + S * S) / R
        A = np.array([seq_sum(y) for y in years[whole]])
        ny = A.size
        amean = np.float64(seq_sum(A)) / np.float64(ny)
        table[16] = amean
        table[17] = np.sqrt(np.float64(seq_sum((A - amean) * (A - amean))) / np.float64(ny - 1)) / amean if ny >= 2 else np.nan
        return table, fdc, regime


def signatures(rows, start=0, nyear=None, cal0=0, probs=None):
    """(table [nrows, 18], fdc [nrows, nP], regime [nrows, 12]) of the windows rows[:, start : start + 12 nyear]."""
    rows = np.asarray(rows, dtype=np.float64)
    probs = probabilities() if probs is None else np.asarray(probs, dtype=np.float64)
    nyear = (rows.shape[1] - start) // 12 if nyear is None else nyear
    out = [signature_row(r[start:start + 12 * nyear], cal0, probs) for r in rows]
    return (np.array([o[0] for o in out]).reshape(len(out), NCOL), np.array([o[1] for o in out]).reshape(len(out), len(probs)),
            np.array([o[2] for o in out]).reshape(len(out), 12))
