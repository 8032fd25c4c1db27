"""What the SPI / SPEI tests share (test_spei_host.py, test_gpu_spei.py): the golden inputs, 40-digit indices and parameters of
the log-logistic distribution (tests/golden/make_golden_spei.py), the restatement's results on them, computed once, and the
error bound.

THE BOUND.  Absolute, in index units, per input and scale: 8 x the error of the numpy restatement (spei_np) against the
40-digit golden on the same elements -- the project's rule for two float64 implementations of one definition (DESIGN 4.18,
sindex_cases).  The restatement's errors as measured on this project's build machines are MEASURED below; the restatement
itself is held to them, the host build of csrc/xh_sindex_dev.h and the device to 8 x them.  What dominates is shared by every
float64 implementation and absent from the golden, whose fit is 40-digit too: the cancellation in 6 w1 - w0 - 6 w2 (the row
shifted by 1e6 has a mean 1e5 times its L-scale; the near-symmetric rows have |beta| of hundreds, i.e. a denominator hundreds
of times smaller than its terms), and exp(beta log z) at those |beta|.  The device's figures stand in test_gpu_spei.py and
DESIGN 4.19."""
import functools
import os

import numpy as np

import sindex_np
import spei_np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SCALES = (1, 3, 12, 24)
INPUTS = (360, 72)
MAX_SHAPE = 1000.0
FACTOR = 8.0
NCELL = 57

# max |restatement - golden| over all non-NaN elements, rounded up to three digits
MEASURED = {
    (360, 1): 9.98e-09, (360, 3): 6.73e-09, (360, 12): 1.59e-09, (360, 24): 2.46e-09,
    (72, 1): 5.62e-10, (72, 3): 1.05e-09, (72, 12): 2.33e-09, (72, 24): 1.42e-10,
}
# Every figure above is met on one row, the one shifted by 1e6, which would leave the other 56 rows four orders of magnitude
# of room.  They are held, in addition, to the restatement's error on them alone (the same rule, the same factor):
SHIFTED_ROW = 12
MEASURED_REST = {
    (360, 1): 9.11e-14, (360, 3): 1.53e-13, (360, 12): 1.57e-13, (360, 24): 2.68e-13,
    (72, 1): 6.38e-14, (72, 3): 6.50e-14, (72, 12): 8.78e-14, (72, 24): 5.78e-15,
}


def bound(n, k, factor=FACTOR):
    return factor * MEASURED[(n, k)]


@functools.lru_cache(maxsize=None)
def _file():
    return np.load(os.path.join(GOLDEN, 'spei.npz'), allow_pickle=False)


def inputs(n):
    """(x [57, n], ref_month0, ref_nyear) of the golden input with n months."""
    f = _file()
    ref = f['ref{}'.format(n)]
    assert tuple(f['scales']) == SCALES
    return f['x{}'.format(n)], int(ref[0]), int(ref[1])


def gold(n, k):
    return _file()['loglogistic_{}_{}'.format(n, k)]


def gold_par(n, k):
    return _file()['par_{}_{}'.format(n, k)]


@functools.lru_cache(maxsize=None)
def restated(n, k):
    """(index, parameters) of the restatement; computed once per process, never modified."""
    x, ref0, nyr = inputs(n)
    idx, par = spei_np.std_index(x, k, ref0, nyr, MAX_SHAPE)
    idx.setflags(write=False)
    par.setflags(write=False)
    return idx, par


def check_against_gold(got, n, k, factor, who):
    """NaN mask identical, every clipped value exactly +-3.09, every element within ``factor`` x MEASURED of the golden (and
    every element outside the shifted row within ``factor`` x MEASURED_REST); returns the two largest errors.  No element is
    left out."""
    limit, limit_rest = factor * MEASURED[(n, k)], factor * MEASURED_REST[(n, k)]
    g = gold(n, k)
    got = np.asarray(got)
    assert got.shape == g.shape
    assert np.array_equal(np.isnan(got), np.isnan(g)), '{} {} {}: NaN masks differ at {}'.format(
        who, n, k, np.argwhere(np.isnan(got) != np.isnan(g))[:5].tolist())
    m = ~np.isnan(g)
    assert np.abs(got[m]).max() <= sindex_np.CLIP
    clipped = m & (np.abs(g) == sindex_np.CLIP)
    assert clipped.any() and np.array_equal(got[clipped], g[clipped]), '{} {} {}: a clipped value is not exactly +-3.09'.format(who, n, k)
    err = np.where(m, np.abs(got - np.where(m, g, 0.0)), 0.0)
    c, t = np.unravel_index(err.argmax(), err.shape)
    worst = float(err[c, t])
    print('{:12s} n={:3d} loglogistic k={:2d}: max |error| {:.3g} at element ({}, {}), bound {:.3g}'.format(who, n, k, worst, c, t, limit))
    assert worst <= limit, '{} {} {}: {:.3g} at element ({}, {}) exceeds {:.3g}'.format(who, n, k, worst, c, t, limit)
    err[SHIFTED_ROW] = 0.0
    c, t = np.unravel_index(err.argmax(), err.shape)
    rest = float(err[c, t])
    print('{:12s} n={:3d} loglogistic k={:2d}: other rows   {:.3g} at element ({}, {}), bound {:.3g}'.format(who, n, k, rest, c, t, limit_rest))
    assert rest <= limit_rest, '{} {} {}: {:.3g} at element ({}, {}) exceeds {:.3g}'.format(who, n, k, rest, c, t, limit_rest)
    return worst, rest


def check_parameters(par, n, k, who):
    """The table against the golden one: the same NaN rows, n exact, alpha / beta / gamma to the cancellation the fit carries
    (relative 1e-6: the golden |beta| keep that distance from the two limits, so it also says 'the same side of them')."""
    g = gold_par(n, k)
    nan_rows = np.isnan(g).any(-1)
    assert np.array_equal(np.isnan(par), np.repeat(nan_rows[..., None], 4, -1)), '{} {} {}: NaN rows differ at {}'.format(
        who, n, k, np.argwhere(np.isnan(par).any(-1) != nan_rows)[:5].tolist())
    assert nan_rows.any() and not nan_rows.all()
    ok = ~nan_rows
    assert np.array_equal(par[ok][:, 3], g[ok][:, 3])
    assert np.allclose(par[ok][:, :3], g[ok][:, :3], rtol=1e-6, atol=0), (who, n, k)
