"""numpy restatement of xh_water_balance (include/xanthos_hip.h, csrc/xh_wbalance_dev.h), row by row, in the stated
order: the 256 strided partial sums joined by the tree of xh_block_sum256 for the S256 and Y256 sums (tests/signatures_np.py),
np.cumsum for the sequential sums, np.sort and the linear rule written out for the medians.  Every column is what the
definition's operations give in IEEE double; only omega and budyko_dev pass through exp, log, log1p and expm1, which come from
numpy's library instead of the compiler's."""
import numpy as np

from signatures_np import quantile, s256, seq_sum

COLUMNS = ('n_years', 'n_months', 'p_mean', 'pet_mean', 'aet_mean', 'q_mean', 'runoff_ratio', 'aridity', 'evaporative', 'residual',
           'closure', 'omega', 'budyko_dev', 'elast_p', 'elast_pet', 'elast_p_ls', 'elast_pet_ls', 'r_pq', 'dry_fraction', 'lag_peak',
           'r_peak')
NCOL = len(COLUMNS)
BISECT = 60
S_LO, S_HI = -13.862943611198906, 4.852030263919617          # log 2^-20, log 2^7, correctly rounded
OMEGA0 = 2.6


def excess(m, lr, omega):
    """m expm1(g(omega)): what Fu's curve lies below min(1, phi) by."""
    with np.errstate(all='ignore'):
        return np.float64(m) * np.expm1(np.log1p(np.exp(np.float64(omega) * lr)) / np.float64(omega))


def fu(phi, omega):
    phi = np.float64(phi)
    if np.isnan(phi):
        return np.float64(np.nan)
    with np.errstate(all='ignore'):
        lo, m = (phi if phi < 1.0 else np.float64(1.0)), (phi if phi > 1.0 else np.float64(1.0))
        return lo - excess(m, np.log(lo / m), omega)


def omega_of(phi, eps):
    """Fu's parameter: 60 bisection steps on s = log(omega - 1), always all of them."""
    phi, eps = np.float64(phi), np.float64(eps)
    with np.errstate(all='ignore'):
        lo, m = (phi if phi < 1.0 else np.float64(1.0)), (phi if phi > 1.0 else np.float64(1.0))
        lr, target = np.log(lo / m), lo - eps
        a, b = np.float64(S_LO), np.float64(S_HI)
        ok = bool(phi == phi and eps > 0.0 and eps < lo)
        ok = ok and bool(target < excess(m, lr, 1.0 + np.exp(a))) and bool(target > excess(m, lr, 1.0 + np.exp(b)))
        for _ in range(BISECT):
            mid = 0.5 * (a + b)
            if excess(m, lr, 1.0 + np.exp(mid)) > target:
                a = mid
            else:
                b = mid
        return np.float64(1.0 + np.exp(0.5 * (a + b))) if ok else np.float64(np.nan)


def balance_row(p, pet, q, aet=None, max_lag=6, omega0=OMEGA0):
    """(table [21], annual [4, nyear], xcorr [max_lag + 1]) of one window of 12 nyear months."""
    with np.errstate(all='ignore'):
        given = [np.asarray(v, dtype=np.float64) + 0.0 for v in (p, pet, q)] + ([np.asarray(aet, dtype=np.float64) + 0.0] if aet is not None else [])
        p, pet, q = given[:3]
        ncol = p.size
        nyear = ncol // 12
        assert ncol == 12 * nyear and nyear >= 1
        inc = np.logical_and.reduce([np.isfinite(v) for v in given])
        table = np.full(NCOL, np.nan)
        annual = np.full((4, nyear), np.nan)
        # the months
        pz, qz = np.where(inc, p, 0.0), np.where(inc, q, 0.0)
        n_months = np.float64(inc.sum())
        mP, mQ = np.float64(s256(pz, inc)) / n_months, np.float64(s256(qz, inc)) / n_months
        dP, dQ = pz - mP, qz - mQ
        den = np.sqrt(np.float64(s256(dP * dP, inc)) * np.float64(s256(dQ * dQ, inc)))
        xcorr = np.full(max_lag + 1, np.nan)
        for k in range(max_lag + 1):
            both = inc[:ncol - k] & inc[k:]
            xcorr[k] = np.float64(s256(dP[:ncol - k] * dQ[k:], both)) / den
        best, at = np.nan, np.nan
        for k in range(max_lag + 1):
            if not np.isnan(xcorr[k]) and not xcorr[k] <= best:
                best, at = xcorr[k], float(k)
        table[1], table[18], table[19], table[20] = n_months, np.float64((inc & (p < pet)).sum()) / n_months, at, best
        # the years
        whole = inc.reshape(nyear, 12).all(axis=1)
        for v, x in enumerate((p, pet, given[3] if aet is not None else None, q)):
            if x is not None:
                annual[v, whole] = [seq_sum(yr) for yr in x.reshape(nyear, 12)[whole]]
        n_years = np.float64(whole.sum())
        table[0] = n_years
        A = np.where(whole, annual, 0.0)
        pbar, petbar, qbar = [np.float64(s256(A[v], whole)) / n_years for v in (0, 1, 3)]
        aetbar = np.float64(s256(A[2], whole)) / n_years if aet is not None else np.float64(np.nan)
        residual = (pbar - aetbar) - qbar
        phi, eps = petbar / pbar, (pbar - qbar) / pbar
        table[2:11] = pbar, petbar, aetbar, qbar, qbar / pbar, phi, aetbar / pbar, residual, residual / pbar
        table[11], table[12] = omega_of(phi, eps), eps - fu(phi, omega0)
        dp, de, dq = A[0] - pbar, A[1] - petbar, A[3] - qbar
        for col, d, bar in ((13, dp, pbar), (14, de, petbar)):
            sel = whole & (d != 0.0)
            if qbar > 0.0 and sel.any():
                table[col] = quantile(np.sort((dq[sel] / d[sel]) * (bar / qbar)), 0.5)
        x1, x2, z = dp / pbar, de / petbar, dq / qbar
        s11, s12, s22, s1z, s2z = [np.float64(s256(t, whole)) for t in (x1 * x1, x1 * x2, x2 * x2, x1 * z, x2 * z)]
        det = s11 * s22 - s12 * s12
        if n_years >= 3 and det > 0.0:
            table[15], table[16] = (s1z * s22 - s2z * s12) / det, (s2z * s11 - s1z * s12) / det
        spq, spp, sqq = [np.float64(s256(t, whole)) for t in (dp * dq, dp * dp, dq * dq)]
        if spp * sqq > 0.0:
            table[17] = spq / np.sqrt(spp * sqq)
        return table, annual, xcorr


def water_balance(p, pet, q, aet=None, start=0, nyear=None, max_lag=6, omega0=OMEGA0):
    """(table [nrows, 21], annual [nrows, 4, nyear], xcorr [nrows, max_lag + 1]) of the windows [:, start : start + 12 nyear]."""
    p, pet, q = [np.asarray(v, dtype=np.float64) for v in (p, pet, q)]
    aet = None if aet is None else np.asarray(aet, dtype=np.float64)
    nyear = (p.shape[1] - start) // 12 if nyear is None else nyear
    w = slice(start, start + 12 * nyear)
    out = [balance_row(p[r, w], pet[r, w], q[r, w], None if aet is None else aet[r, w], max_lag, omega0) for r in range(p.shape[0])]
    return (np.array([o[0] for o in out]).reshape(len(out), NCOL), np.array([o[1] for o in out]).reshape(len(out), 4, nyear),
            np.array([o[2] for o in out]).reshape(len(out), max_lag + 1))
