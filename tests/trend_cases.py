"""The rows the trend tests run on, shared by tests/test_trend_host.py, tests/test_gpu_trend.py and
tests/golden/make_golden_trend.py: for every shape (nseason 1 and 12; 4, 5, 22, 64, 65 and 257 years) rows of every kind in
turn, row r of kind KINDS[r % len(KINDS)], drawn from a fixed seed."""
import numpy as np

NSEASONS = (1, 12)
YEARS = (4, 5, 22, 64, 65, 257)
SHAPES = [(ns, ny) for ns in NSEASONS for ny in YEARS]
KINDS = ('random', 'tied', 'constant', 'increasing', 'decreasing', 'signed_zeros', 'scattered_nan', 'season_nan', 'few',
         'infinities', 'trend_with_ties', 'random_wide')
HOST_ROWS = 2 * len(KINDS)            # every kind twice
Z95 = -1.959963984540054              # scipy.stats.norm.ppf(0.025)
TINY = 2.3e-308                       # below it p is only asked to lie in [0, TINY]


def make_rows(nseason, years, nrows, seed=0):
    ncol = nseason * years
    rng = np.random.default_rng(1000 * years + 10 * nseason + seed)
    rows = np.empty((nrows, ncol))
    t = np.arange(ncol, dtype=np.float64)
    for r in range(nrows):
        kind = KINDS[r % len(KINDS)]
        x = rng.gamma(2.0, 3.0, ncol)
        if kind == 'tied':
            x = np.floor(x / 4.0)
        elif kind == 'constant':
            x[:] = (0.0, 7.25)[(r // len(KINDS)) % 2]
        elif kind == 'increasing':
            x = np.cumsum(x + 0.001)
        elif kind == 'decreasing':
            x = -np.cumsum(x + 0.001)
        elif kind == 'signed_zeros':
            x = np.where(rng.random(ncol) < 0.6, np.where(rng.random(ncol) < 0.5, 0.0, -0.0), np.round(x - 6.0))
        elif kind == 'scattered_nan':
            x[rng.random(ncol) < 0.15] = np.nan
        elif kind == 'season_nan':
            x[int(rng.integers(nseason))::nseason] = np.nan
        elif kind == 'few':
            keep = rng.choice(ncol, size=int(rng.integers(0, 4)), replace=False)
            y = np.full(ncol, np.nan)
            y[keep] = x[keep]
            x = y
        elif kind == 'infinities':
            x[rng.random(ncol) < 0.1] = np.inf
            x[rng.random(ncol) < 0.1] = -np.inf
        elif kind == 'trend_with_ties':
            x = np.round(x + 0.02 * t / nseason)
        elif kind == 'random_wide':
            x = (x - 6.0) * 10.0 ** rng.integers(-8, 9, ncol)
        rows[r] = x
    return rows


def same_but_p(a, b):
    """Nine columns equal in value (==: the sign of a zero is free) and identical NaN masks, column 4 (p) aside."""
    a, b = np.asarray(a), np.asarray(b)
    cols = [c for c in range(10) if c != 4]
    return (np.array_equal(np.isnan(a), np.isnan(b))
            and np.array_equal(a[:, cols], b[:, cols], equal_nan=True))


def p_within(p, ref, bound):
    """p against the reference: both NaN, or 0 <= p <= TINY where the reference lies below TINY, or within ``bound``
    (relative)."""
    p, ref = np.asarray(p), np.asarray(ref)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(p), nan):
        return False
    tiny = ~nan & (ref < TINY)
    rest = ~nan & ~tiny
    return bool(((p[tiny] >= 0.0) & (p[tiny] <= TINY)).all() and (np.abs(p[rest] - ref[rest]) <= bound * ref[rest]).all())
