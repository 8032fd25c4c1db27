"""The numpy restatement of the bootstrap of xanthos_amd/csrc/xh_exboot_dev.h: the draws in np.uint64
arithmetic, the resampled series built explicitly and sorted, and the fit with extremes_np's functions -- so the sums of a
replicate are the header's bits (the same weights, the same order over the sorted sample) and k and the levels agree to the
rounding of expm1, log and Gamma.  The intervals are np.quantile(method='linear') of the replicates that have a fit."""
import numpy as np

import extremes_np

NREP = 5                         # l1, l2, t3, t4, k before a replicate's levels
MAX_B = 2048
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def row_key(seed, rows):
    with np.errstate(over='ignore'):
        return splitmix64(np.uint64(seed) ^ (np.asarray(rows).astype(np.uint64) * np.uint64(0xD1342543DE82EF95)))


def draws(seed, rows, reps, n):
    """j_i [len(rows), len(reps), n] of the rows (their numbers row0 + r) and the replicates ``reps``."""
    h_rep = splitmix64(row_key(seed, rows)[:, None] ^ (np.asarray(reps).astype(np.uint64) + np.uint64(1))[None, :])
    m = np.arange((n + 1) // 2, dtype=np.uint64) + np.uint64(1)
    word = splitmix64(h_rep[:, :, None] ^ m[None, None, :])
    u = np.stack([word & np.uint64(0xFFFFFFFF), word >> np.uint64(32)], axis=3).reshape(word.shape[0], word.shape[1], -1)[:, :, :n]
    return ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def replicate_fits(samples, return_periods):
    """samples [m, n] (no NaN) -> [m, 5 + nT]: l1, l2, t3, t4 as computed, k and the levels (NaN without a fit)."""
    n, l1, l2, t3, t4, varies = extremes_np.lmoments(samples)
    with np.errstate(invalid='ignore'):
        fit = varies & (l2 > 0.0) & (t3 <= extremes_np.T3_MAX)
    k = np.where(fit, extremes_np.k_of_t3(np.where(fit, t3, 0.0)), np.nan)
    with np.errstate(invalid='ignore'):
        fit &= (k > -1.0) & np.isfinite(k)
    k = np.where(fit, k, np.nan)
    alpha, xi = extremes_np.gev_parameters(l1, l2, k)
    return np.stack([l1, l2, t3, t4, k] + [extremes_np.quantile(T, k, alpha, xi) for T in return_periods], axis=1)


def intervals(rep, B, confidence, kind):
    """rep [B, 5 + nT] of one row with a fit -> its ci row [3 + 2 nT]."""
    fit = ~np.isnan(rep[:, 4])
    nb = int(fit.sum())
    nq = rep.shape[1] - 4
    out = np.full(1 + 2 * nq, np.nan)
    out[0] = nb
    if 2 * nb >= B:
        p_lo = (1.0 - confidence) / 2.0
        p_hi = 1.0 - p_lo
        for q in range(nq):
            lo, hi = np.quantile(rep[fit, 4 + q], [p_lo, p_hi], method='linear')
            out[1 + 2 * q], out[2 + 2 * q] = (-hi, -lo) if kind == 'min' and q > 0 else (lo, hi)
    return out


def bootstrap_rows(x, kind, return_periods, B, confidence, seed, row0=0, min_years=10, start=0, nyear=None, fits=replicate_fits):
    """(ci [nrows, 3 + 2 nT], rep [nrows, B, 5 + nT]) of the window x[:, start : start + 12 nyear]; ``fits``: what turns the
    sorted samples [m, n] into [m, 5 + nT] (the golden file's 40-digit one instead of numpy's)."""
    x = np.asarray(x, dtype=np.float64)
    nyear = (x.shape[1] - start) // 12 if nyear is None else nyear
    nT = len(return_periods)
    table, annual, _ = extremes_np.extremes_rows(x, kind, (), min_years=min_years, start=start, nyear=nyear)
    z = (-annual if kind == 'min' else annual)
    zs = np.sort(z, axis=1, kind='stable')
    ci = np.full((x.shape[0], 3 + 2 * nT), np.nan)
    ci[:, 0] = 0.0
    rep = np.full((x.shape[0], B, NREP + nT), np.nan)
    fitted = ~np.isnan(table[:, 5])
    counts = table[:, 0].astype(np.int64)
    for n in np.unique(counts[fitted]):
        rows = np.flatnonzero(fitted & (counts == n))
        for at in range(0, rows.size, 64):
            some = rows[at:at + 64]
            j = draws(seed, row0 + some, np.arange(B), int(n))
            samples = np.sort(zs[some][np.arange(some.size)[:, None, None], j], axis=2)        # [rows, B, n]
            rep[some] = fits(samples.reshape(-1, int(n)), return_periods).reshape(some.size, B, -1)
    for r in np.flatnonzero(fitted):
        ci[r] = intervals(rep[r], B, confidence, kind)
    return ci, rep
