"""Golden values of the standardized drought indices: the definitions of xh_std_index evaluated with mpmath at
40 digits on two small inputs, from the float64 accumulated series X of the restatement (tests/sindex_np.py) -- the sums of the
fit, log, the incomplete gamma function and the inverse normal are all 40-digit here, so what is left between a float64
implementation and these values is that implementation's own error.

    python tests/golden/make_golden_sindex.py        (a few minutes on 8 cores)

writes tests/golden/sindex.npz (both inputs, their reference periods, and the indices of the [70, 360] input) and
tests/golden/sindex_72.npz (the indices of the [70, 72] input; one file would pass the size limit for a committed file).
Arrays: x360, x72; ref360, ref72 = (ref_month0, ref_nyear); scales; gamma_<n>_<k>, empirical_<n>_<k> for n in 360, 72.

Rows of the inputs (70 cells: more than one wave, not a multiple of 64): a seeded seasonal gamma field, and
    3, 4   35 % zeros                 5   scaled by 1e-3              6   all zero
    7      3 positive values per calendar month (the rest zero)
    8      nearly constant: alpha ~ 1e8 exceeds max_shape              9, 12   alpha of a few hundred
    10     one NaN                    11  one negative value
The [70, 360] input takes years 5 - 24 as its reference period, so months outside it exercise in = 0 and values beyond every
sample (clipping); the [70, 72] input its whole six years (n = 6 per calendar month, 4 - 5 at scale 24).
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import sindex_np  # noqa: E402

mp.mp.dps = 40
SCALES = (1, 3, 12, 24)
MAX_SHAPE = 1000.0
CLIP = 3.09
LIMIT = 1 << 20


def make_input(nmonths, seed):
    rng = np.random.default_rng(seed)
    ncell = 70
    season = 1.0 + 0.6 * np.sin(2 * np.pi * (np.arange(nmonths) % 12) / 12.0 + rng.uniform(0, 6.28, (ncell, 1)))
    shape = rng.uniform(0.6, 6.0, (ncell, 1))
    x = rng.gamma(shape, 10.0 / shape, (ncell, nmonths)) * season
    for r in (3, 4):
        x[r, rng.random(nmonths) < 0.35] = 0.0
    x[5] *= 1e-3
    x[6] = 0.0
    keep = np.zeros(nmonths, dtype=bool)
    nyear = nmonths // 12
    for y in ((5, 10, 15) if nyear >= 16 else (1, 3, 4)):
        keep[12 * y:12 * y + 12] = True
    x[7, ~keep] = 0.0
    x[8] = 100.0 * (1.0 + 1e-4 * rng.standard_normal(nmonths))
    x[9] = rng.gamma(300.0, 0.1, nmonths)
    x[12] = rng.gamma(600.0, 0.05, nmonths)
    x[10, nmonths // 3 + 1] = np.nan
    x[11, nmonths // 2 + 5] = -0.25
    # values a float32 holds exactly: half the bytes of the stored input are zero, and nothing about the test changes
    return x.astype(np.float32).astype(np.float64)


def mp_ndtri_clipped(H):
    if H != H:
        return float('nan')
    if H < mp.mpf('0.0009'):            # ndtri(0.001) = -3.0902...
        return -CLIP
    if H > mp.mpf('0.9991'):
        return CLIP
    z = mp.sqrt(2) * mp.erfinv(2 * H - 1)
    return float(min(max(z, -CLIP), CLIP))


def mp_fit(sample):
    """(q0, alpha, beta) at 40 digits or None."""
    s = [float(v) for v in sample]
    if any(v != v or v < 0 for v in s):
        return None
    pos = [mp.mpf(v) for v in s if v > 0]
    if len(pos) < 4:
        return None
    q0 = mp.mpf(sum(1 for v in s if v == 0)) / len(s)
    mu = mp.fsum(pos) / len(pos)
    ml = mp.fsum(mp.log(v) for v in pos) / len(pos)
    A = mp.log(mu) - ml
    if not A > 0:
        return None
    alpha = (1 + mp.sqrt(1 + 4 * A / 3)) / (4 * A)
    if alpha > MAX_SHAPE:
        return None
    return q0, alpha, mu / alpha


def gamma_row(args):
    Xrow, k, ref0, nyr = args
    nmonths = Xrow.size
    out = np.full(nmonths, np.nan)
    for m in range(12):
        u = sindex_np.sample_months(nmonths, k, ref0, nyr, m)
        fit = mp_fit(Xrow[u])
        if fit is None:
            continue
        q0, alpha, beta = fit
        for t in range(m, nmonths, 12):
            X = float(Xrow[t])
            if X != X or X < 0:
                continue
            H = q0 if X == 0 else q0 + (1 - q0) * mp.gammainc(alpha, 0, mp.mpf(X) / beta, regularized=True)
            out[t] = mp_ndtri_clipped(H)
    return out


def empirical_row(args):
    Xrow, k, ref0, nyr = args
    nmonths = Xrow.size
    out = np.full(nmonths, np.nan)
    for m in range(12):
        s = Xrow[sindex_np.sample_months(nmonths, k, ref0, nyr, m)]
        n = s.size
        if np.isnan(s).any() or n < 4:
            continue
        for t in range(m, nmonths, 12):
            X = Xrow[t]
            if X != X:
                continue
            in_ref = 1 if ref0 <= t < ref0 + 12 * nyr else 0
            L, E = int((s < X).sum()), int((s == X).sum())
            rank = mp.mpf(2 * L + E + 2 - in_ref) / 2
            out[t] = mp_ndtri_clipped((rank - mp.mpf('0.44')) / (n + 1 - in_ref + mp.mpf('0.12')))
    return out


def main():
    x360, x72 = make_input(360, 20241), make_input(72, 20242)
    ref = {360: (60, 20), 72: (0, 6)}
    big = dict(x360=x360, x72=x72, ref360=np.array(ref[360]), ref72=np.array(ref[72]), scales=np.array(SCALES))
    small = {}
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for n, x, dest in ((72, x72, small), (360, x360, big)):
            for k in SCALES:
                X = sindex_np.accumulate(x, k)
                rows = [(X[c], k, ref[n][0], ref[n][1]) for c in range(X.shape[0])]
                dest['gamma_{}_{}'.format(n, k)] = np.array(pool.map(gamma_row, rows, chunksize=1))
                dest['empirical_{}_{}'.format(n, k)] = np.array(pool.map(empirical_row, rows, chunksize=1))
                print(n, k, 'done', flush=True)
    for name, arrays in (('sindex.npz', big), ('sindex_72.npz', small)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(name, size, 'bytes')
        assert size < LIMIT, '{} is {} bytes: over the limit for a committed file'.format(name, size)


if __name__ == '__main__':
    main()
