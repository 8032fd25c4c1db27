"""Golden values of the log-logistic standardized index (SPI / SPEI): the definitions of xh_std_index2 evaluated
with mpmath at 40 digits on two small inputs, from the float64 accumulated series X of the restatement (tests/sindex_np.py's
``accumulate``) -- the sort is exact, the three sums, beta, g, alpha, gamma, log, exp and the inverse normal are all 40-digit
here, so what is left between a float64 implementation and these values is that implementation's own error.

    python tests/golden/make_golden_spei.py        (under a minute on 8 cores)

writes tests/golden/spei.npz: x360, x72; ref360, ref72 = (ref_month0, ref_nyear); scales; loglogistic_<n>_<k> [57, n] and
par_<n>_<k> [57, 12, 4] = (alpha, beta, gamma, n) for n in 360, 72 and k in 1, 3, 12, 24.

Rows of the inputs (57 cells).  The field is a climatic water balance: a seeded
seasonal gamma field minus a near-constant seasonal demand, positively skewed, negative about half the time.  Then
    3, 4   precipitation-like: no demand, 35 % zeros (ties)      5    scaled by 1e-3          6   constant (2.5)
    7      negative skew (the mirrored field)
    8      symmetric about its calendar month's mean over the reference years to ~1e-7: |beta| far beyond max_shape at scale 1
    9, 15  near-symmetric (normal): |beta| of tens to hundreds    10   one NaN
    11     rounded to whole numbers in a narrow range (many ties)  12   shifted by 1e6
    13     positive skew, the months after the reference period far BELOW the fitted support: exactly -3.09
    14     negative skew, the months after the reference period far ABOVE the fitted support: exactly +3.09
The [70, 360] input takes years 5 - 24 as its reference period; the [70, 72] input its first five years, which leaves n = 3 at
scale 24 in eleven calendar months (NaN) and n = 4 in December.

Two conditions keep NaN masks and exact clips comparable between this file and any float64 implementation, and are asserted
here: no unclipped golden value lies within MARGIN of +-3.09, and no golden |beta| lies within 1e-6 relative of 1 or of
max_shape.
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
MARGIN = 1e-6            # far above every bound the tests hold an implementation to
NCELL = 57          # (70 as in sindex.npz would pass that file's size, the limit set for this one: few of these rows are NaN)


def make_input(nmonths, seed, ref):
    rng = np.random.default_rng(seed)
    nyear = nmonths // 12
    ref_y0, ref_nyr = ref[0] // 12, ref[1]
    mon = np.arange(nmonths) % 12
    season = 1.0 + 0.6 * np.sin(2 * np.pi * mon / 12.0 + rng.uniform(0, 6.28, (NCELL, 1)))
    shape = rng.uniform(0.6, 6.0, (NCELL, 1))
    precip = rng.gamma(shape, 10.0 / shape, (NCELL, nmonths)) * season
    demand = 9.0 * (1.0 + 0.5 * np.sin(2 * np.pi * mon / 12.0 + 1.0)) * (1.0 + 0.02 * rng.standard_normal((NCELL, nmonths)))
    x = precip - demand
    for r in (3, 4):
        x[r] = precip[r]
        x[r, rng.random(nmonths) < 0.35] = 0.0
    x[5] *= 1e-3
    x[6] = 2.5
    x[7] = 4.0 - x[7]
    # row 8: calendar month's mean + a year effect whose values over the reference years are +-d_1 .. +-d_(nyr/2) (and 0)
    d = rng.uniform(1.0, 10.0, ref_nyr // 2)
    effect = np.concatenate([d, -d, np.zeros(ref_nyr % 2)])
    rng.shuffle(effect)
    year_effect = rng.uniform(-10.0, 10.0, nyear)
    year_effect[ref_y0:ref_y0 + ref_nyr] = effect
    x[8] = 64.0 + 8.0 * np.sin(2 * np.pi * mon / 12.0) + np.repeat(year_effect, 12)
    x[9] = 20.0 + 5.0 * rng.standard_normal(nmonths)
    x[15] = -3.0 + 2.0 * rng.standard_normal(nmonths)
    x[10, nmonths // 3 + 1] = np.nan
    x[11] = np.round(rng.gamma(2.0, 1.5, nmonths)) - 2.0
    x[12] += 1e6
    after = 12 * (ref_y0 + ref_nyr)
    x[14] = 4.0 - x[14]
    x[13, after:] = x[13, :after].min() - 60.0
    x[14, after:] = x[14, :after].max() + 60.0
    # values a float32 holds exactly: half the bytes of the stored input are zero, and nothing about the test changes
    return x.astype(np.float32).astype(np.float64)


def mp_ndtri_clipped(H):
    if H < mp.mpf('0.0009'):            # ndtri(0.001) = -3.0902...
        return -CLIP
    if H > mp.mpf('0.9991'):
        return CLIP
    z = mp.sqrt(2) * mp.erfinv(2 * H - 1)
    return float(min(max(z, -CLIP), CLIP))


def mp_fit(sample):
    """(alpha, beta, gamma) at 40 digits, or None."""
    s = sorted(float(v) for v in sample)
    n = len(s)
    if n < 4 or any(v != v for v in sample) or s[0] == s[-1]:
        return None
    v = [mp.mpf(x) for x in s]
    w0 = mp.fsum(v) / n
    w1 = mp.fsum(v[i - 1] * mp.mpf(n - i) / (n - 1) for i in range(1, n + 1)) / n
    w2 = mp.fsum(v[i - 1] * mp.mpf((n - i) * (n - i - 1)) / ((n - 1) * (n - 2)) for i in range(1, n + 1)) / n
    den = 6 * w1 - w0 - 6 * w2
    if den == 0:
        return None                      # beta infinite
    beta = (2 * w1 - w0) / den
    if beta == 0:
        return None
    g = (mp.pi / beta) / mp.sin(mp.pi / beta) if abs(beta) > 1 else None
    for edge in (1.0, MAX_SHAPE):
        assert abs(abs(beta) / edge - 1) > 1e-6, 'a golden |beta| = {} lies next to {}'.format(beta, edge)
    if not 1 < abs(beta) <= MAX_SHAPE:
        return None
    alpha = (w0 - 2 * w1) * beta / g
    return alpha, beta, w0 - alpha * g


def row(args):
    Xrow, k, ref0, nyr = args
    nmonths = Xrow.size
    out = np.full(nmonths, np.nan)
    par = np.full((12, 4), np.nan)
    for m in range(12):
        s = Xrow[sindex_np.sample_months(nmonths, k, ref0, nyr, m)]
        fit = mp_fit(s)
        if fit is None:
            continue
        alpha, beta, gamma = fit
        par[m] = float(alpha), float(beta), float(gamma), float(s.size)
        for t in range(m, nmonths, 12):
            X = float(Xrow[t])
            if X != X:
                continue
            z = (mp.mpf(X) - gamma) / alpha
            H = (mp.mpf(0) if alpha > 0 else mp.mpf(1)) if z <= 0 else 1 / (1 + mp.exp(-beta * mp.log(z)))
            out[t] = mp_ndtri_clipped(H)
    return out, par


def main():
    ref = {360: (60, 20), 72: (0, 5)}
    # (seeds at which the two asserted conditions hold: with seed 20252 a five-year sample of a row with 35 % zeros is four
    # zeros and one value, whose beta is exactly 1)
    x360, x72 = make_input(360, 20251, ref[360]), make_input(72, 20253, ref[72])
    arrays = dict(x360=x360, x72=x72, ref360=np.array(ref[360]), ref72=np.array(ref[72]), scales=np.array(SCALES))
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for n, x in ((72, x72), (360, x360)):
            for k in SCALES:
                X = sindex_np.accumulate(x, k)
                res = pool.map(row, [(X[c], k, ref[n][0], ref[n][1]) for c in range(NCELL)], chunksize=1)
                g = arrays['loglogistic_{}_{}'.format(n, k)] = np.array([r[0] for r in res])
                arrays['par_{}_{}'.format(n, k)] = np.array([r[1] for r in res])
                near = np.abs(np.abs(g[~np.isnan(g)]) - CLIP)
                assert not ((near > 0) & (near < MARGIN)).any(), 'an unclipped golden value lies within {} of the clip'.format(MARGIN)
                print(n, k, 'done: {:.1%} NaN, {} clipped low, {} clipped high'.format(
                    np.isnan(g).mean(), int((g == -CLIP).sum()), int((g == CLIP).sum())), flush=True)
    # the rows the tests count on
    for n in (360, 72):
        g, par = arrays['loglogistic_{}_1'.format(n)], arrays['par_{}_1'.format(n)]
        after = ref[n][0] + 12 * ref[n][1]
        assert np.isnan(g[[6, 8]]).all()
        # (a five-year sample may come out near-symmetric, and then no value lies outside its support)
        assert (g[13, after:] == -CLIP).mean() > 0.7 and (g[14, after:] == CLIP).mean() > 0.7
        assert (par[7, :, 1] < 0).sum() > (par[7, :, 1] > 0).sum() and (par[0, :, 1] > 0).sum() > (par[0, :, 1] < 0).sum()
    assert np.isnan(arrays['par_72_24'][:, :11]).all() and not np.isnan(arrays['par_72_24'][:, 11]).all()
    path = os.path.join(HERE, 'spei.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    limit = os.path.getsize(os.path.join(HERE, 'sindex.npz'))
    print('spei.npz', size, 'bytes')
    assert size <= limit, 'spei.npz is {} bytes: larger than sindex.npz ({})'.format(size, limit)


if __name__ == '__main__':
    main()
