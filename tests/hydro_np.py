"""Numpy restatements of xanthos/hydropower/potential.py and actual.py, written from the reference's semantics and the
summation orders of pandas / numpy, vectorised over cells or dams.  Used by test_hydro_host.py
(against the reference's golden vectors) and test_gpu_hydro.py (against the kernels at full size)."""
import numpy as np
import pandas as pd

SWW, HOURS, TWH, EJ = 9810, 730.5, 10 ** -12, 0.0036
SECS, MM3, HOURS_YEAR, MWH_EJ = 2629800, 2.6298, 8766, 3.6 * (10 ** -9)


def kahan_rows(x, labels, nlab):
    """pandas' compensated group sum over the rows of ``x`` [n, k] (row order, NaN skipped): (sums, counts) [nlab, k]."""
    k = x.shape[1]
    s, c, n = np.zeros((nlab, k)), np.zeros((nlab, k)), np.zeros((nlab, k), dtype=np.int64)
    for i in range(x.shape[0]):
        g = labels[i]
        v = x[i]
        ok = ~np.isnan(v)
        y = v - c[g]
        t = s[g] + y
        cc = (t - s[g]) - y
        cc[np.isnan(cc)] = 0.0
        s[g] = np.where(ok, t, s[g])
        c[g] = np.where(ok, cc, c[g])
        n[g] += ok
    return s, n


def _leaf(a):
    n = a.shape[0]
    if n < 8:
        r = np.full(a.shape[1:], -0.0)
        for i in range(n):
            r = r + a[i]
        return r
    r = [a[j].copy() for j in range(8)]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] = r[j] + a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + a[i]
        i += 1
    return res


def pairwise_sum(a):
    """np.add.reduce along axis 0 of a 1-D slice, per column of ``a``: numpy's pairwise summation."""
    def rec(a):
        n = a.shape[0]
        if n <= 128:
            return _leaf(a)
        n2 = n // 2
        n2 -= n2 % 8
        return rec(a[:n2]) + rec(a[n2:])
    return 0.0 + rec(a)


def years_of(start, nmonths):
    years = np.asarray(pd.period_range(start, periods=nmonths, freq='M').year)
    uniq, idx = np.unique(years, return_inverse=True)
    return idx, uniq


def potential_cells(q, elev, q_ex, ef, start):
    """(q_max [ncell], E [ncell, nyears]) of potential.py:27-46."""
    q_max = np.percentile(q, q_ex * 100, axis=1)
    qc = np.clip(q, 0, q_max[:, None])
    e = ((((ef * SWW) * qc) * HOURS) * TWH) * np.asarray(elev, dtype=np.float64)[:, None]
    idx, uniq = years_of(start, q.shape[1])
    s, _ = kahan_rows(e.T, idx, len(uniq))
    return q_max, s.T * EJ


def region_sums(E, keys):
    """groupby(keys, axis=1).sum() of E [ncell, nyears] -> (sorted keys, sums [ngroups, nyears])."""
    uniq, inv = np.unique(keys, return_inverse=True)
    s, _ = kahan_rows(E, inv, len(uniq))
    return uniq, s


def env_flow(inflow, start):
    """env_flow_constraint (actual.py:109-117) for every dam: inflow [nmonths, ndams] -> [ndams, 12]."""
    nm = inflow.shape[0]
    m0 = pd.Period(start, freq='M').month - 1
    month = (m0 + np.arange(nm)) % 12
    s, n = kahan_rows(inflow, month, 12)
    mmf = s / n
    maf = pairwise_sum(inflow) / nm
    lo, hi = 0.4 * maf, 0.8 * maf
    p = (np.where(mmf < lo, 0.6, 0.0) + np.where((mmf >= lo) & (mmf <= hi), 0.45, 0.0)
         + np.where(mmf > hi, 0.3 * np.where(mmf < 1, 0.0, 1.0), 0.0))
    return (p * mmf).T


def dam_parameters(res):
    cap = res['CAP'].values.astype(float)
    cap_live = np.where(np.isnan(res['CAPLIVE'].values), cap, res['CAPLIVE'].values).astype(float)
    q_max = res['FLOW_M3S'].values * MM3
    eff = res['EFF'].values.astype(float)
    head = res['HEAD'].values.astype(float)
    fb = res['ECAP'].values / (eff * SWW * (q_max / SECS))
    return cap, cap_live, q_max, eff, np.where(np.isnan(head), fb, head)


def march(inflow, env, rc, params, start):
    """get_power (actual.py:124-145) for every dam: power [nmonths, ndams] (Python's min / max as written)."""
    cap, cap_live, q_max, eff, head = params
    rc = np.where(np.isnan(rc), 1.1, rc)
    nm, nd = inflow.shape
    m0 = pd.Period(start, freq='M').month - 1
    breaks = np.linspace(0, 1, 5)
    s = cap.copy()
    power = np.empty((nm, nd))
    cols = np.arange(nd)

    def pmin(a, b):
        return np.where(b < a, b, a)

    def pmax(a, b):
        return np.where(b > a, b, a)
    for t in range(nm):
        m = (m0 + t) % 12
        s_state = s / cap
        active = s + inflow[t] - (cap - cap_live)
        ok = rc[:, m, :] <= s_state[None, :]
        assert ok.any(axis=0).all(), 'no rule-curve row <= s / cap'
        last = 4 - np.argmax(ok[::-1], axis=0)
        release = breaks[last] * q_max
        r = pmin(pmin(pmax(release, env[cols, m]), active), q_max)
        s1 = pmax(pmin(s + inflow[t] - r, cap), 0.0)
        h = ((0.0 + (s + s1)) / 2 / cap) * head
        power[t] = pmax(eff * SWW * h * (r / SECS), 0.0)
        s = s1
    return power


def annual_means(power, start):
    idx, uniq = years_of(start, power.shape[0])
    s, n = kahan_rows(power, idx, len(uniq))
    return s / n
