"""numpy / pandas restatements of the diagnostics' summation orders, for tests only.

pairwise_rows : numpy's pairwise_sum along each row (loops_utils.h.src), spelled out: < 8 values left to right, <= 128
                values in eight accumulators folded ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus the tail, longer rows split at
                n/2 rounded down to a multiple of 8; rows longer than 8192 values are summed in blocks of 8192 added
                one after the other, from 0.0.  Vectorised over the rows.
kahan_groups  : pandas' groupby sum (groupby.pyx group_sum): per group, cells in ascending order, NaN skipped, compensated,
                the compensation reset to 0 when it turns NaN.  Vectorised over the groups.
aggregation   : time_series.py:Aggregation_Map -- per id > 0, cells in ascending order from 0.0, NaN skipped.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from xanthos_amd.diagnostics.diagnostics import COLUMNS, scale_table, scatter_table  # noqa: E402


def _pairwise(a):
    n = a.shape[1]
    if n < 8:
        res = np.zeros(a.shape[0])
        for i in range(n):
            res = res + a[:, i]
        return res
    if n <= 128:
        r = [a[:, j].copy() for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + a[:, i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for k in range(i, n):
            res = res + a[:, k]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:, :n2]) + _pairwise(a[:, n2:])


def pairwise_rows(a):
    """np.sum(a, axis=1): the reduction's inner loop sees blocks of at most 8192 values (the ufunc buffer size), summed
    pairwise and added to the running total one after the other from 0.0."""
    a = np.asarray(a, dtype=float)
    res = np.zeros(a.shape[0])
    for off in range(0, a.shape[1], 8192):
        res = res + _pairwise(a[:, off:off + 8192])
    return res


def cell_totals(Q, nyear, area):
    """diagnostics.py:58: np.sum(Q, axis=1) / nyear * area / 1e6."""
    return pairwise_rows(Q) / nyear * area / 1e6


def kahan_groups(vals, ids):
    """(sorted unique ids, [ngroups, k] compensated sums, counts) of the [ncell, k] values."""
    vals = np.asarray(vals, dtype=float)
    vals = vals.reshape(vals.shape[0], -1)
    uniq, inv = np.unique(np.asarray(ids), return_inverse=True)
    order = np.argsort(inv, kind='stable')
    counts = np.bincount(inv, minlength=len(uniq))
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    s = np.zeros((len(uniq), vals.shape[1]))
    c = np.zeros_like(s)
    with np.errstate(invalid='ignore'):
        for j in range(int(counts.max()) if len(counts) else 0):
            g = np.flatnonzero(counts > j)
            v = vals[order[start[g] + j]]
            ok = ~np.isnan(v)
            y = v - c[g]
            t = s[g] + y
            cn = (t - s[g]) - y
            cn[np.isnan(cn)] = 0.0
            s[g] = np.where(ok, t, s[g])
            c[g] = np.where(ok, cn, c[g])
    return uniq, s, counts


def aggregation(ids, data):
    """[max(id), ncols] table of time_series.py:Aggregation_Map."""
    ids = np.asarray(ids).astype(np.int64)
    data = np.asarray(data, dtype=float)
    table = np.zeros((int(ids.max()), data.shape[1]))
    keep = ids > 0
    # adding +0.0 for a NaN equals skipping it: the running sum starts at +0.0 and never becomes -0.0
    np.add.at(table, ids[keep] - 1, np.where(np.isnan(data[keep]), 0.0, data[keep]))
    return table


def diag_tables(Q, nyear, ref, scales=('Basin', 'Country', 'Region')):
    """The three csv tables of Diagnostics, with the orders above (pandas only formats them)."""
    ncell = Q.shape[0]
    vals = np.zeros((ncell, len(COLUMNS)))
    vals[:, 0] = cell_totals(Q, nyear, ref.area)
    vals[:, 1] = pairwise_rows(ref.vic) / ref.vic.shape[1]
    vals[:, 2] = scatter_table(ref.wbmd, ncell, 'WBM')
    vals[:, 3] = scatter_table(ref.wbmc, ncell, 'WBMc')
    vals[:, 4] = ref.unh
    out = {}
    for sc, attr, off in (('Basin', 'basin', 1), ('Country', 'country', 0), ('Region', 'region', 1)):
        if sc in scales:
            uniq, sums, _ = kahan_groups(vals, getattr(ref, attr + '_ids'))
            out[sc] = scale_table(uniq, sums, getattr(ref, attr + '_names'), off)
    return out
