"""The rows the signature tests share (tests/test_signatures_host.py, tests/test_gpu_signatures.py, the golden values of
tests/golden/make_golden_signatures.py): one row of every kind at every year count, from fixed seeds."""
import numpy as np

# years: 1 the smallest window; 21 / 22 under and just over one pass of the 256 lanes (252 / 264 columns); 43 and 86 over a power
# of two (516 / 1032 columns); 341 the limit (4092 columns)
YEARS = (1, 2, 5, 21, 22, 43, 86, 341)
KINDS = ('skewed', 'seasonal', 'intermittent', 'constant', 'all_nan', 'scattered', 'year_nan', 'one_finite', 'two_finite',
         'month_nan', 'shifted', 'negative', 'signed_zeros', 'ascending', 'descending')
CAL0 = 3            # the window starts in April: the calendar months are not the columns mod 12
EXCEEDANCE = (1, 5, 10, 20, 50, 80, 90, 95, 99)


def row(kind, nyear):
    ncol = 12 * nyear
    rng = np.random.default_rng(7000 + 97 * KINDS.index(kind) + nyear)
    t = np.arange(ncol)
    season = 1.0 + 0.8 * np.sin(2.0 * np.pi * (t % 12) / 12.0)
    x = np.round(np.exp(rng.normal(1.0, 1.2, ncol)) * season, 6)          # skewed positive flow
    if kind == 'seasonal':
        x = np.round(50.0 * season ** 4 + rng.uniform(0.0, 0.5, ncol), 6)
    elif kind == 'intermittent':
        x = np.where(rng.random(ncol) < 0.6, 0.0, np.round(x, 0))
    elif kind == 'constant':
        x = np.full(ncol, 3.7)
    elif kind == 'all_nan':
        x = np.full(ncol, np.nan)
    elif kind == 'scattered':
        hit = rng.random(ncol)
        x = np.where(hit < 0.08, np.nan, np.where(hit < 0.12, np.inf, np.where(hit < 0.16, -np.inf, x)))
    elif kind == 'year_nan':
        y = nyear // 2
        x[12 * y:12 * y + 12] = np.nan
    elif kind == 'one_finite':
        keep = int(rng.integers(ncol))
        x = np.where(t == keep, x, np.nan)
    elif kind == 'two_finite':
        keep = rng.choice(ncol, 2, replace=False)
        x = np.where(np.isin(t, keep), x, np.nan)
    elif kind == 'month_nan':
        x = np.where(t % 12 == 5, np.nan, x)
    elif kind == 'shifted':
        x = x + 1.0e6
    elif kind == 'negative':
        x = np.round(rng.normal(0.0, 5.0, ncol), 6)
    elif kind == 'signed_zeros':
        x = np.where(rng.random(ncol) < 0.3, -0.0, np.where(rng.random(ncol) < 0.3, 0.0, x))
    elif kind == 'ascending':
        x = np.sort(x)
    elif kind == 'descending':
        x = np.sort(x)[::-1]
    return np.ascontiguousarray(x, dtype=np.float64)


def rows(nyear):
    """[len(KINDS), 12 nyear]: one row of every kind."""
    return np.stack([row(kind, nyear) for kind in KINDS])
