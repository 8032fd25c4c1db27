"""The rows the extreme-value tests run on, shared by tests/test_extremes_host.py, tests/test_gpu_extremes.py and
tests/golden/make_golden_extremes.py: for every year count rows of every kind in turn, row r of kind KINDS[r % len(KINDS)],
drawn from a fixed seed; and the error measures the golden file records and the tests bound."""
import numpy as np

YEARS = (5, 10, 50, 63, 64, 65, 129, 341)        # (the wave boundary; 341 years = 4092 columns, the end of the limit)
KINDS = ('gev_-0.4', 'gev_-0.2', 'gev_0', 'gev_0.2', 'gev_0.4', 'gev_0.6', 'ties', 'constant', 'all_nan', 'scattered_nan',
         'year_nan', 'few', 'shifted', 'negative', 'signed_zeros')
HOST_ROWS = 2 * len(KINDS)                       # every kind twice
MIN_YEARS = 5
GOLDEN_T = (2.0, 10.0, 100.0, 1000.0)
CLASSES = ('ordinary', 'shifted')
QUANTITIES = ('lmom', 'k', 'alpha', 'xi', 'level', 'T_year')
K_FLOOR = 0.03125                                # k: absolute error below this |k| (as a relative one at it), relative above
EPS = float(np.finfo(np.float64).eps)


def kind_of(r):
    return KINDS[r % len(KINDS)]


def class_of(r):
    return 'shifted' if kind_of(r) == 'shifted' else 'ordinary'


def gev_sample(rng, k, n, xi=40.0, alpha=12.0):
    u = -np.log(rng.random(n))
    return xi - alpha * np.log(u) if k == 0.0 else xi + alpha * (1.0 - u ** k) / k


def make_rows(nyear, nrows, seed=0):
    rng = np.random.default_rng(100 * nyear + seed)
    rows = np.empty((nrows, 12 * nyear))
    for r in range(nrows):
        kind = kind_of(r)
        k = float(kind[4:]) if kind.startswith('gev_') else 0.1
        # the year's largest month is a GEV sample; the others lie below it by gamma-distributed amounts
        top = gev_sample(rng, k, nyear)
        m = top[:, None] - rng.gamma(2.0, 6.0, (nyear, 12))
        m[np.arange(nyear), rng.integers(0, 12, nyear)] = top
        if kind == 'ties':
            wet = rng.random(nyear) < 0.3
            m = np.where(wet[:, None] & (rng.random((nyear, 12)) < 0.3), np.abs(m), 0.0)
        elif kind == 'constant':
            m[:] = (0.0, 7.25)[(r // len(KINDS)) % 2]
        elif kind == 'all_nan':
            m[:] = np.nan
        elif kind == 'scattered_nan':
            m[rng.random((nyear, 12)) < 0.02] = np.nan
            m[rng.random((nyear, 12)) < 0.005] = np.inf
        elif kind == 'year_nan':
            m[int(rng.integers(nyear))] = np.nan
        elif kind == 'few':
            keep = rng.choice(nyear, size=int(rng.integers(0, MIN_YEARS)), replace=False)
            gone = np.ones(nyear, dtype=bool)
            gone[keep] = False
            m[gone, rng.integers(0, 12, int(gone.sum()))] = np.nan
        elif kind == 'shifted':
            m = m + 1.0e6
        elif kind == 'negative':
            m = m - 150.0
        elif kind == 'signed_zeros':
            m = np.where(rng.random((nyear, 12)) < 0.7, np.where(rng.random((nyear, 12)) < 0.5, 0.0, -0.0), np.round(m / 8.0))
        rows[r] = m.ravel()
    return rows


def lmom_error(lm, ref):
    """l1, l2, t3, t4 [nrows, 4] against the reference's: the largest of |dl1| / max(|l1|, l2) (l1 passes through 0),
    |dl2| / l2, |dt3| and |dt4| (ratios inside [-1, 1])."""
    lm, ref = np.asarray(lm), np.asarray(ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        d = np.abs(lm - ref)
        return np.max([d[:, 0] / np.maximum(np.abs(ref[:, 0]), ref[:, 1]), d[:, 1] / ref[:, 1], d[:, 2], d[:, 3]], axis=0)


def errors(table, T_year, ref_table, ref_T_year):
    """{quantity: [nrows] the largest error of the row in the quantity's measure, NaN for a row without a fit}.  lmom: see
    lmom_error.  k: |dk| /
    max(|k|, K_FLOOR).  alpha is l2 times a factor d / Gamma(1 + k) that falls to 0 like 1 + k as k -> -1, where Gamma(1 + k)
    magnifies the rounding of k by 1 / (1 + k) in alpha's RELATIVE error while its error relative to l2 stays that of k: it is
    taken against the larger of alpha and l2 (for k > -0.6 that is alpha itself).  xi and the return levels are sums of l1 and multiples of l2, so their error is taken
    against the largest of |value|, |l1| and l2 (xi itself passes through 0).  T_y: relative, over the finite ones."""
    table, ref_table = np.asarray(table), np.asarray(ref_table)
    with np.errstate(invalid='ignore', divide='ignore'):
        fit = ~np.isnan(ref_table[:, 5])
        out = {'k': np.abs(table[:, 5] - ref_table[:, 5]) / np.maximum(np.abs(ref_table[:, 5]), K_FLOOR),
               'alpha': np.abs(table[:, 6] - ref_table[:, 6]) / np.maximum(ref_table[:, 6], ref_table[:, 2])}
        out['lmom'] = np.where(fit, lmom_error(table[:, 1:5], ref_table[:, 1:5]), np.nan)
        scale = np.maximum(np.abs(ref_table[:, 1]), ref_table[:, 2])[:, None]
        loc = np.abs(table[:, 7:] - ref_table[:, 7:]) / np.maximum(np.abs(ref_table[:, 7:]), scale)
        out['xi'] = loc[:, 0]
        out['level'] = loc[:, 1:].max(axis=1) if loc.shape[1] > 1 else np.where(fit, 0.0, np.nan)
        fin = np.isfinite(ref_T_year) & np.isfinite(T_year)
        rel = np.where(fin, np.abs(T_year - ref_T_year) / np.where(fin, ref_T_year, 1.0), 0.0)
        out['T_year'] = np.where(fit, rel.max(axis=1), np.nan)
    return out


def sweep_errors(k, alpha, xi, ref_k, ref_alpha, ref_xi):
    """The pieces over the t3 sweep (alpha and xi for l1 = 0, l2 = 1) in the same measures: xi / l2 passes through 0 at k = 1
    and is taken against the larger of itself and alpha / l2, alpha / l2 against the larger of itself and 1."""
    return {'k': np.abs(k - ref_k) / np.maximum(np.abs(ref_k), K_FLOOR), 'alpha': np.abs(alpha - ref_alpha) / np.maximum(ref_alpha, 1.0),
            'xi': np.abs(xi - ref_xi) / np.maximum(np.abs(ref_xi), ref_alpha)}


def same_masks(table, annual, T_year, ref_table, ref_annual, ref_T_year):
    """Identical NaN masks everywhere, identical n, and T_y infinite where the reference's is."""
    return (np.array_equal(np.isnan(table), np.isnan(ref_table)) and np.array_equal(np.isnan(annual), np.isnan(ref_annual))
            and np.array_equal(np.isnan(T_year), np.isnan(ref_T_year)) and np.array_equal(table[:, 0], ref_table[:, 0])
            and np.array_equal(np.isinf(T_year), np.isinf(ref_T_year)))


def bits_equal(table, annual, ref_table, ref_annual):
    """n, l1, l2, t3, t4 and the annual series bit for bit (the sign of a zero included; a NaN is a NaN)."""
    def bits(a):
        a = np.ascontiguousarray(a)
        return np.isnan(a).tobytes() + np.where(np.isnan(a), 0.0, a).tobytes()
    return bits(table[:, :5]) == bits(ref_table[:, :5]) and bits(annual) == bits(ref_annual)
