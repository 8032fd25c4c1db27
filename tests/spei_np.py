"""numpy restatement of the log-logistic standardized index (SPI / SPEI and the distribution of DESIGN 4.19; the definitions
of xh_std_index2 in include/xanthos_hip.h), per cell and calendar month as a user would write it behind a download: np.sort,
the three sums in the order the definition gives.  Test infrastructure only: the product never imports it.  The accumulated
series, the sample months and the clip are those of sindex_np.

    fit_sample(s, max_shape)               (alpha, beta, gamma, n) of one sample in any order, or four NaNs
    cdf(X, alpha, beta, gamma)             H of one value (or arrays)
    fit(X, k, ref0, nyr, max_shape)        parameters [ncell, 12, 4]
    index(X, par)                          index [ncell, nmonths]
    std_index(x, k, ref0, nyr, max_shape=1000.0, par=None, minus=None) -> (index, par)
"""
import math

import numpy as np
from scipy.special import ndtri

from sindex_np import CLIP, accumulate, sample_months

BAD = (np.nan,) * 4


def fit_sample(s, max_shape=1000.0):
    s = np.asarray(s, dtype=np.float64)
    n = s.size
    if n < 4 or np.isnan(s).any():
        return BAD
    s = np.sort(s)
    if s[0] == s[-1]:                                       # a constant sample: 0 / 0 in exact arithmetic
        return BAD
    s0 = s1 = s2 = 0.0
    d1, d2 = float(n - 1), float((n - 1) * (n - 2))
    for i in range(1, n + 1):                               # s_1 the smallest; python floats: one rounding per operation
        v = float(s[i - 1])
        s0 = s0 + v
        s1 = s1 + v * (float(n - i) / d1)
        s2 = s2 + v * (float((n - i) * (n - i - 1)) / d2)
    w0, w1, w2 = s0 / n, s1 / n, s2 / n
    with np.errstate(all='ignore'):
        beta = np.float64(2.0 * w1 - w0) / np.float64(6.0 * w1 - w0 - 6.0 * w2)
        pb = np.float64(math.pi) / beta
        g = pb / np.sin(pb)
        alpha = (w0 - 2.0 * w1) * beta / g
        gamma = w0 - alpha * g
    if not (np.isfinite(alpha) and np.isfinite(beta) and np.isfinite(gamma)) or not 1.0 < abs(beta) <= max_shape:
        return BAD
    return float(alpha), float(beta), float(gamma), float(n)


def cdf(X, alpha, beta, gamma):
    """H; NaN where X or a parameter is NaN."""
    X, alpha, beta, gamma = np.broadcast_arrays(*[np.asarray(v, dtype=np.float64) for v in (X, alpha, beta, gamma)])
    ok = ~(np.isnan(X) | np.isnan(alpha) | np.isnan(beta) | np.isnan(gamma))
    with np.errstate(all='ignore'):
        z = (X - gamma) / alpha
        ok = ok & ~np.isnan(z)
        inside = ok & (z > 0)
        H = 1.0 / (1.0 + np.exp(-beta * np.log(np.where(inside, z, 1.0))))
        H = np.where(inside, H, np.where(alpha > 0, 0.0, 1.0))
    return np.where(ok, H, np.nan)


def fit(X, k, ref0, nyr, max_shape=1000.0):
    ncell, nmonths = X.shape
    par = np.full((ncell, 12, 4), np.nan)
    for m in range(12):
        u = sample_months(nmonths, k, ref0, nyr, m)
        for c in range(ncell):
            par[c, m] = fit_sample(X[c, u], max_shape)
    return par


def index(X, par):
    nmonths = X.shape[1]
    p = par[:, np.arange(nmonths) % 12, :]
    H = cdf(X, p[..., 0], p[..., 1], p[..., 2])
    with np.errstate(all='ignore'):
        return np.clip(ndtri(H), -CLIP, CLIP)


def std_index(x, k, ref0, nyr, max_shape=1000.0, par=None, minus=None):
    x = np.asarray(x, dtype=np.float64)
    if minus is not None:
        x = x - np.asarray(minus, dtype=np.float64)
    X = accumulate(x, k)
    if par is None:
        par = fit(X, k, ref0, nyr, max_shape)
    return index(X, par), par
