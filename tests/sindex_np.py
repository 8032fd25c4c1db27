"""numpy / scipy restatement of the standardized drought indices (the definitions of xh_std_index in
include/xanthos_hip.h), per cell and calendar month as a user would write it behind a download.  Test infrastructure only:
the product never imports it.

    accumulate(x, k)                       X [ncell, nmonths]
    sample_months(nmonths, k, ref0, nyr, m)  the months u of R(., m)
    fit_gamma(X, k, ref0, nyr, max_shape)  parameters [ncell, 12, 4] = (q0, alpha, beta, n)
    index_gamma(X, par)                    index [ncell, nmonths]
    index_empirical(X, k, ref0, nyr)       index [ncell, nmonths]
    std_index(x, k, ref0, nyr, dist, max_shape=1000.0, par=None) -> (index, par or None)
"""
import numpy as np
from scipy.special import gammainc, ndtri

CLIP = 3.09


def accumulate(x, k):
    """X[c, t] = ((x[c, t-k+1] + x[c, t-k+2]) + ...) + x[c, t], left to right; NaN for t < k - 1."""
    x = np.asarray(x, dtype=np.float64)
    X = np.full(x.shape, np.nan)
    n = x.shape[1]
    if k <= n:
        acc = x[:, 0:n - k + 1].copy()
        for j in range(1, k):
            acc = acc + x[:, j:n - k + 1 + j]
        X[:, k - 1:] = acc
    return X


def sample_months(nmonths, k, ref0, nyr, m):
    u = np.arange(ref0 + m, ref0 + 12 * nyr, 12)
    return u[u >= k - 1]


def _seq_sum(values):
    s = 0.0
    for v in values:
        s = s + v
    return s


def fit_gamma_sample(s, max_shape=1000.0):
    """(q0, alpha, beta, n) of one sample in ascending month order, or four NaNs."""
    bad = (np.nan,) * 4
    s = np.asarray(s, dtype=np.float64)
    n = s.size
    if np.isnan(s).any() or (s < 0).any():
        return bad
    pos = s[s > 0]
    if pos.size < 4:
        return bad
    q0 = float(np.count_nonzero(s == 0)) / n
    mu = _seq_sum(pos) / pos.size
    ml = _seq_sum(np.log(pos)) / pos.size
    A = np.log(mu) - ml
    if not A > 0:
        return bad
    alpha = (1.0 + np.sqrt(1.0 + 4.0 * A / 3.0)) / (4.0 * A)
    if alpha > max_shape:
        return bad
    return q0, alpha, mu / alpha, float(n)


def fit_gamma(X, k, ref0, nyr, max_shape=1000.0):
    ncell, nmonths = X.shape
    par = np.full((ncell, 12, 4), np.nan)
    for m in range(12):
        u = sample_months(nmonths, k, ref0, nyr, m)
        for c in range(ncell):
            par[c, m] = fit_gamma_sample(X[c, u], max_shape)
    return par


def index_gamma(X, par):
    ncell, nmonths = X.shape
    p = par[:, np.arange(nmonths) % 12, :]                      # [ncell, nmonths, 4]
    q0, alpha, beta = p[..., 0], p[..., 1], p[..., 2]
    ok = ~(np.isnan(X) | (X < 0) | np.isnan(q0) | np.isnan(alpha) | np.isnan(beta))
    with np.errstate(all='ignore'):
        Xs = np.where(ok, X, 1.0)
        H = q0 + (1.0 - q0) * gammainc(np.where(ok, alpha, 1.0), Xs / np.where(ok, beta, 1.0))
        H = np.where(Xs == 0, q0, H)
        z = np.clip(ndtri(H), -CLIP, CLIP)
    return np.where(ok, z, np.nan)


def empirical_position(X, sample, in_ref):
    """The Gringorten probability of one value against one sample (brute-force counts), or NaN."""
    sample = np.asarray(sample, dtype=np.float64)
    n = sample.size
    if np.isnan(X) or np.isnan(sample).any() or n < 4:
        return np.nan
    L = int(np.count_nonzero(sample < X))
    E = int(np.count_nonzero(sample == X))
    N = n + 1 - in_ref
    rank = L + (E + 2 - in_ref) / 2.0
    return (rank - 0.44) / (N + 0.12)


def index_empirical(X, k, ref0, nyr):
    ncell, nmonths = X.shape
    out = np.full(X.shape, np.nan)
    for m in range(12):
        u = sample_months(nmonths, k, ref0, nyr, m)
        for c in range(ncell):
            s = X[c, u]
            for t in range(m, nmonths, 12):
                in_ref = 1 if ref0 <= t < ref0 + 12 * nyr else 0
                p = empirical_position(X[c, t], s, in_ref)
                out[c, t] = np.nan if np.isnan(p) else min(max(ndtri(p), -CLIP), CLIP)
    return out


def std_index(x, k, ref0, nyr, dist, max_shape=1000.0, par=None):
    X = accumulate(x, k)
    if dist == 'empirical':
        return index_empirical(X, k, ref0, nyr), None
    if par is None:
        par = fit_gamma(X, k, ref0, nyr, max_shape)
    return index_gamma(X, par), par
