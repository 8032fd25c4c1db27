"""The numpy restatement of the extreme-value definition of xanthos_amd/csrc/xh_extremes_dev.h, vectorised over
the rows: annual maxima or minima of a monthly window, Hosking's unbiased sample L-moments, the GEV fitted by them, return
levels and each year's return period.  Every operation stands in the header's order -- the sums run over ascending rank from
0.0, w_r(i) = (w_{r-1}(i) (i - r + 1)) / (n - r), nothing is contracted --, so n, the annual series, l1, l2, t3 and t4 are the
header's bits; k, alpha, xi, the return levels and T_y go through numpy's and scipy's expm1, log1p, exp, log and gamma and
agree with the header's to those functions' rounding."""
import numpy as np
from scipy import special

COLUMNS = ('n', 'l1', 'l2', 't3', 't4', 'k', 'alpha', 'xi')
NPAR = len(COLUMNS)
KINDS = ('max', 'min')
NEWTON_STEPS = 10
K_SERIES = 0.25                  # below it (1 - Gamma(1 + k)) / k comes from the Taylor series of Gamma(1 + k)
K_DLOG_SERIES = 0.0078125        # below it Newton's d log f / dk comes from its series
T3_MAX = 1.0 - 2.0 ** -20        # above it no fit: k <= -1, decided on t3
LN2 = 0.6931471805599453094
LN3 = 1.0986122886681096914
EULER = 0.57721566490153286061
# Gamma(1 + x) = 1 + sum_j GAMMA_TAYLOR[j - 1] x^j, j = 1 .. 30 (40-digit values, rounded once)
GAMMA_TAYLOR = (
    -0.57721566490153286061, 0.9890559953279725554, -0.90747907608088628902, 0.98172808683440018734, -0.9819950689031452021,
    0.99314911462127619315, -0.99600176044243153397, 0.99810569378312892198, -0.99902526762195486779, 0.99951565607277744107,
    -0.99975659750860128703, 0.99987827131513327573, -0.99993906420644431684, 0.9999695177634821045, -0.99998475269937704874,
    0.99999237447907321586, -0.99999618658947331203, 0.99999809308113089205, -0.99999904646891115772, 0.99999952321060573958,
    -0.99999976159734438057, 0.99999988079601916842, -0.99999994039712498375, 0.99999997019826758236, -0.99999998509903547505,
    0.99999999254948496246, -0.99999999627473155544, 0.99999999813736213559, -0.99999999906867985371, 0.99999999953433952215)


def annual_series(x, kind):
    """[nrows, 12 nyear] -> [nrows, nyear]: the largest (smallest) of the year's 12 months by comparisons from the first month
    on (v > a replaces a: of equal months the first stays); NaN where a month is NaN or +-inf."""
    x = np.asarray(x, dtype=np.float64)
    m = x.reshape(x.shape[0], -1, 12)
    a = m[:, :, 0].copy()
    for j in range(1, 12):
        v = m[:, :, j]
        with np.errstate(invalid='ignore'):
            a = np.where((v > a) if kind == 'max' else (v < a), v, a)
    a[~np.isfinite(m).all(axis=2)] = np.nan
    return a


def lmoments(z):
    """z [nrows, nyear] with NaN for a missing year -> n, l1, l2, t3, t4 (each [nrows]; NaN where not defined) and whether the
    series is not constant."""
    z = np.asarray(z, dtype=np.float64)
    nrows, nyear = z.shape
    valid = ~np.isnan(z)
    n = valid.sum(axis=1)
    zs = np.sort(z, axis=1, kind='stable')                    # NaNs last
    nf = n.astype(np.float64)
    b = np.zeros((4, nrows))
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(nyear):
            live = i < n
            zi = np.where(live, zs[:, i], 0.0)
            w = np.ones(nrows)
            for r in range(4):
                if r:
                    w = (w * float(i - r + 1)) / (nf - float(r))
                b[r] = np.where(live & (n > r), b[r] + w * zi, b[r])
        b = b / nf
        for r in range(4):
            b[r] = np.where(n > r, b[r], np.nan)
        l1 = b[0]
        l2 = 2.0 * b[1] - b[0]
        l3 = (6.0 * b[2] - 6.0 * b[1]) + b[0]
        l4 = ((20.0 * b[3] - 30.0 * b[2]) + 12.0 * b[1]) - b[0]
        t3, t4 = l3 / l2, l4 / l2
        varies = zs[:, 0] < zs[np.arange(nrows), np.maximum(n, 1) - 1]
    return nf, l1, l2, t3, t4, varies


def _f_of_k(k):
    with np.errstate(all='ignore'):
        A, B = np.expm1(-k * LN3), np.expm1(-k * LN2)
        f = np.where(k == 0.0, LN3 / LN2, A / B)
        series = (-(LN3 - LN2) / 2.0 + ((LN3 * LN3 - LN2 * LN2) / 12.0) * k) - ((LN3 ** 4 - LN2 ** 4) / 720.0) * ((k * k) * k)
        direct = (LN2 * (B + 1.0)) / B - (LN3 * (A + 1.0)) / A
        return f, np.where(np.abs(k) < K_DLOG_SERIES, series, direct)


def k_of_t3(t3, steps=NEWTON_STEPS, trace=None):
    """The root k of (1 - 3^-k) / (1 - 2^-k) = (3 + t3) / 2 by `steps` Newton steps from Hosking's start."""
    t3 = np.asarray(t3, dtype=np.float64)
    with np.errstate(all='ignore'):
        target = (3.0 + t3) / 2.0
        c = 2.0 / (3.0 + t3) - LN2 / LN3
        k = 7.8590 * c + (2.9554 * c) * c
        for _ in range(steps):
            f, dlog = _f_of_k(k)
            k = k - (f - target) / (f * dlog)
            if trace is not None:
                trace.append(k.copy())
    return k


def gamma1_over_k(k, gam):
    """(1 - Gamma(1 + k)) / k: the series below K_SERIES, the quotient from gam = Gamma(1 + k) elsewhere."""
    k = np.asarray(k, dtype=np.float64)
    p = np.full(k.shape, GAMMA_TAYLOR[-1])
    for cj in GAMMA_TAYLOR[-2::-1]:
        p = p * k + cj
    with np.errstate(all='ignore'):
        return np.where(np.abs(k) < K_SERIES, -p, (1.0 - gam) / k)


def gev_parameters(l1, l2, k):
    """alpha, xi of the GEV with L-moments l1, l2 and shape k."""
    l1, l2, k = (np.asarray(v, dtype=np.float64) for v in (l1, l2, k))
    with np.errstate(all='ignore'):
        gam = special.gamma(1.0 + k)
        d = np.where(k == 0.0, 1.0 / LN2, k / -np.expm1(-k * LN2))
        alpha = (l2 * d) / gam
        xi = l1 - alpha * gamma1_over_k(k, gam)
    return alpha, xi


def quantile(T, k, alpha, xi):
    """The value of z exceeded once in T years on average."""
    with np.errstate(all='ignore'):
        ly = np.log(-np.log1p(-1.0 / np.float64(T)))
        return np.where(k == 0.0, xi - alpha * ly, xi - alpha * (np.expm1(k * ly) / k))


def return_period(z, k, alpha, xi):
    """T = 1 / (1 - F(z)) under the GEV: 1 at F = 0, +inf at F = 1."""
    with np.errstate(all='ignore'):
        s = (z - xi) / alpha
        t = -k * s
        u = np.where(k == 0.0, np.exp(-s), np.where(t <= -1.0, np.where(k > 0.0, 0.0, np.inf), np.exp(np.log1p(t) / k)))
        T = -1.0 / np.expm1(-u)
        return np.where(np.isnan(s) | np.isnan(k), np.nan, T)


def extremes_rows(x, kind, return_periods, min_years=10, start=0, nyear=None, parameters=None):
    """(table [nrows, 8 + nT], annual [nrows, nyear], T_year [nrows, nyear]) of the window x[:, start : start + 12 nyear]."""
    x = np.asarray(x, dtype=np.float64)
    nyear = (x.shape[1] - start) // 12 if nyear is None else nyear
    a = annual_series(x[:, start:start + 12 * nyear], kind)
    sign = -1.0 if kind == 'min' else 1.0
    z = sign * a
    nT = len(return_periods)
    nan = np.full(x.shape[0], np.nan)
    if parameters is None:
        n, l1, l2, t3, t4, varies = lmoments(z)
        with np.errstate(invalid='ignore'):
            fit = (n >= min_years) & varies & (l2 > 0.0) & (t3 <= T3_MAX)
        k = np.where(fit, k_of_t3(np.where(fit, t3, 0.0)), np.nan)
        with np.errstate(invalid='ignore'):
            fit &= (k > -1.0) & np.isfinite(k)
        alpha, xi = gev_parameters(l1, l2, np.where(fit, k, np.nan))
        t3, t4, k = (np.where(fit, v, nan) for v in (t3, t4, k))
        par = np.stack([n, sign * l1, l2, t3, t4, k, alpha, sign * xi], axis=1)
    else:
        par = np.array(np.asarray(parameters, dtype=np.float64)[:, :NPAR])
        k, alpha, xi = par[:, 5], par[:, 6], sign * par[:, 7]
    levels = [sign * quantile(T, k, alpha, xi) for T in return_periods]
    table = np.concatenate([par] + [np.asarray(q, dtype=np.float64)[:, None] for q in levels], axis=1)
    T_year = return_period(z, k[:, None], alpha[:, None], xi[:, None])
    return table, a, T_year
