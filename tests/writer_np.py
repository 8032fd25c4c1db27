"""Hostile inputs for the output writer's sums and pandas' own reductions, for tests only.

``hostile(rng, ncell, nmonths)`` gives [ncell, nmonths] values where the summation order shows: mixed signs over many
decades, -0.0, subnormals and NaN sprinkled everywhere, and special years placed on the first cells (year k of cell k,
cycling through the years): an exact cancellation whose plain left-to-right sum is 8.0 and whose compensated sum is
10.0, NaN first / last / alone, an all-NaN year, a lone +inf, a lone -inf, +inf with -inf, an overflow to inf, -0.0
only and subnormals only.  Later cells repeat the special years at random places.
"""
import numpy as np

CANCEL = [1e16, 1.0, 1.0, -1e16] + [1.0] * 8          # pandas: 10.0, a plain sum: 8.0
NAN, INF = np.nan, np.inf
SPECIAL = [
    CANCEL,
    [NAN, 1e16, 1.0, -1e16, 1.0, 3e-5, 1.0, -7.0, 1.0, 1.0, 1.0, 1.0],           # NaN first
    [1e16, 1.0, 1.0, -1e16, 1.0, 3e-5, 1.0, -7.0, 1.0, 1.0, 1.0, NAN],           # NaN last
    [NAN] * 5 + [2.5] + [NAN] * 6,                                              # one value alone among NaN
    [1e-3, 2e3, -5e8, 1.0, 1e8, NAN, 4e8, 7.0, -1e-7, 3.0, 2.0, 1.0],           # one NaN alone among values
    [NAN] * 12,                                                                 # all-NaN year
    [1.0, 2.0, INF, 3.0, -1e300, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 1e-300],         # lone +inf
    [1.0, -INF, 2.0, 3.0, 4.0, 1e300, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0],           # lone -inf
    [1.0, INF, 2.0, 3.0, 4.0, 5.0, -INF, 6.0, 7.0, 8.0, 9.0, 10.0],             # +inf and -inf
    [1.5e308, 1.5e308, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0],      # overflow to inf
    [-0.0] * 12,                                                                # -0.0 only
    [5e-324, -1e-310, 3e-320, 2.2e-308, -2.2e-308, 1e-315, 7e-322, 0.0, -0.0, 1e-320, -5e-324, 4e-309],  # subnormals
]


def hostile(rng, ncell, nmonths):
    assert nmonths % 12 == 0
    nyear = nmonths // 12
    q = rng.standard_normal((ncell, nmonths)) * 10.0 ** rng.integers(-12, 17, (ncell, nmonths))
    r = rng.random((ncell, nmonths))
    q[r < 0.04] = np.nan
    q[(r >= 0.04) & (r < 0.06)] = -0.0
    sub = (r >= 0.06) & (r < 0.08)
    q[sub] = rng.integers(-4000, 4000, int(sub.sum())) * 5e-324
    for k in range(min(ncell, len(SPECIAL))):
        y = k % nyear
        q[k, 12 * y:12 * y + 12] = SPECIAL[k]
    for c in range(len(SPECIAL), ncell, 7):            # the special years again, at random places
        y = int(rng.integers(nyear))
        q[c, 12 * y:12 * y + 12] = SPECIAL[int(rng.integers(len(SPECIAL)))]
    return q


def pandas_agg_to_year(q, func):
    """pandas' groupby 'sum' / 'mean' over blocks of 12 columns (the reduction OutWriter.agg_to_year makes)."""
    import pandas as pd
    return pd.DataFrame(q).T.groupby(np.arange(q.shape[1]) // 12).agg(func).T.values


def pandas_agg_spatial(q, id_map, n_ids, first_id):
    """pandas' groupby('id').sum() of the cells (the reduction OutWriter.agg_spatial makes), one row per id
    first_id .. first_id + n_ids - 1; NaN for an id without cells."""
    import pandas as pd
    sums = pd.DataFrame(q).groupby(np.asarray(id_map)).sum()
    return sums.reindex(np.arange(first_id, first_id + n_ids)).values.astype(float)
