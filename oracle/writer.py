"""Output aggregation (oracle; test infrastructure only).

numpy restatement of the array math of xanthos/data_writer/out_writer.py: agg_to_year (:237-248), the mm -> km3
conversion in write() (:111-112, rows x area / 1e6) and agg_spatial (:250-265).

Both aggregations are pandas groupby reductions, and pandas (2.x, groupby.pyx group_sum / group_mean) adds with a
compensated (Kahan) update, in ascending column order for agg_to_year and ascending cell order for agg_spatial:

    for each value v:  if v is NaN: skip
                       y = v - c;  t = s + y;  c = (t - s) - y;  if c is NaN: c = 0;  s = t;  n += 1
    sum -> s (all-NaN -> 0.0)        mean -> s / n (n == 0 -> NaN)

The NaN reset of c keeps a lone +/-inf infinite; +inf and -inf together give NaN.  Ids without cells give NaN rows
(left merge of the names, :261); ids outside the names are dropped.
"""
import numpy as np


def _kahan(vals, ok):
    """Compensated sums over the leading axis of ``vals`` (values where ``ok`` is False are skipped): (s, n)."""
    s = np.zeros(vals.shape[1:])
    c = np.zeros_like(s)
    n = np.zeros(vals.shape[1:], dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for v, m in zip(vals, ok):
            y = v - c
            t = s + y
            cn = (t - s) - y
            cn[np.isnan(cn)] = 0.0
            s = np.where(m, t, s)
            c = np.where(m, cn, c)
            n += m
    return s, n


def agg_to_year(arr, func='sum'):
    """[ncell, nmonths] -> [ncell, nmonths // 12]: pandas' compensated sum or mean of each block of 12 columns."""
    arr = np.asarray(arr, dtype=float)
    a = arr.reshape(arr.shape[0], -1, 12).transpose(2, 0, 1)          # [12, ncell, nyears]
    s, n = _kahan(a, ~np.isnan(a))
    if func == 'sum':
        return s
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(n > 0, s / np.maximum(n, 1), np.nan)


def mm_to_km3(arr, grid_areas):
    return np.asarray(arr, dtype=float) * (np.asarray(grid_areas, dtype=float) / 1e6)[:, None]


def agg_spatial(arr, id_map, n_ids, first_id=1):
    """Rows = ids first_id .. first_id + n_ids - 1 (the reference's names table): per id, pandas' compensated sum over its
    cells in ascending order; NaN where an id has no cells."""
    arr = np.asarray(arr, dtype=float)
    arr = arr.reshape(arr.shape[0], -1)
    k = np.asarray(id_map).reshape(-1).astype(np.int64) - first_id
    keep = np.flatnonzero((k >= 0) & (k < n_ids))
    k = k[keep]
    counts = np.bincount(k, minlength=n_ids)
    out = np.full((n_ids, arr.shape[1]), np.nan)
    if not len(k):
        return out
    # step j adds the j-th cell (ascending) of every id that has more than j cells
    order = keep[np.argsort(k, kind='stable')]
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    s = np.zeros((n_ids, arr.shape[1]))
    c = np.zeros_like(s)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(int(counts.max())):
            g = np.flatnonzero(counts > j)
            v = arr[order[start[g] + j]]
            y = v - c[g]
            t = s[g] + y
            cn = (t - s[g]) - y
            cn[np.isnan(cn)] = 0.0
            m = ~np.isnan(v)
            s[g] = np.where(m, t, s[g])
            c[g] = np.where(m, cn, c[g])
    out[counts > 0] = s[counts > 0]
    return out
