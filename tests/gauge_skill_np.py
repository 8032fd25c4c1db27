"""The skill of routed streamflow at stream gauges in numpy: what xh_gauge_skill is held to.

Per gauge, over the months V whose observation is finite (n = |V|, s = flow[cell, V], o = obs[V]): n, ED through
oracle.calib.kge_distance (the reference's Kling-Gupta distance, calibrate_abcd.py:196-213), its three components as that
function forms them, and NSE, PBIAS and RMSE from their formulas as written.  n < 2, or a NaN flow at a month of V, gives
NaN in every column but the first."""
import numpy as np

from oracle.calib import kge_distance

COLS = ('n', 'ed', 'r', 'alpha', 'beta', 'nse', 'pbias', 'rmse')


def gauge_row(series, obs):
    """The eight columns of one gauge: ``series`` [nmonths] (the flow of its cell), ``obs`` [nmonths], NaN = missing."""
    series, obs = np.asarray(series, dtype=float), np.asarray(obs, dtype=float)
    v = np.isfinite(obs)
    s, o = series[v], obs[v]
    n = int(v.sum())
    if n < 2 or np.isnan(s).any():
        return np.array([n] + [np.nan] * 7)
    with np.errstate(all='ignore'):
        ed = float(kge_distance(s, o))
        r = float(np.clip(np.corrcoef(o, s)[1, 0], -1.0, 1.0))
        alpha = np.std(s) / np.std(o)
        beta = np.mean(s) / np.mean(o)
        nse = 1.0 - np.sum((s - o) ** 2) / np.sum((o - np.mean(o)) ** 2)
        pbias = 100.0 * np.sum(s - o) / np.sum(o)
        rmse = np.sqrt(np.sum((s - o) ** 2) / n)
    return np.array([n, ed, r, alpha, beta, nse, pbias, rmse])


def skill(flow, cells, obs):
    """[ngauge, 8] of ``flow`` [ncell, nmonths] at the 0-based cells ``cells`` against ``obs`` [ngauge, nmonths]."""
    flow = np.asarray(flow)
    return np.stack([gauge_row(flow[int(c)], o) for c, o in zip(cells, obs)])


def table(raw):
    """[..., 8] -> {column of gauge_skill.csv: array}: months_used, kge = 1 - ED, r, alpha, beta, nse, pbias, rmse."""
    raw = np.asarray(raw)
    out = {'months_used': raw[..., 0].astype(np.int64), 'kge': 1.0 - raw[..., 1]}
    for j, name in enumerate(('r', 'alpha', 'beta', 'nse', 'pbias', 'rmse'), start=2):
        out[name] = raw[..., j]
    return out
