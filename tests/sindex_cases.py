"""What the standardized-index tests share (test_sindex_host.py, test_gpu_sindex.py): the golden inputs and 40-digit indices
(tests/golden/make_golden_sindex.py), the restatement's results on them, computed once, and the error bound.

THE BOUND.  Absolute, in index units, per input, distribution and scale: 8 x the error of the numpy / scipy restatement
(sindex_np) against the 40-digit golden on the same elements.  The restatement's errors as measured (scipy 1.x gammainc / ndtri
on this project's build machines) are MEASURED below; the restatement itself is held to them, the host build of
csrc/xh_sindex_dev.h and the device to 8 x them.  What dominates the gamma figures is shared by every float64 implementation:
the cancellation in A = log(mu) - ml, which the golden does not have (its fit is 40-digit too) -- the worst elements are the
rows with a shape of several hundred, where A ~ 1 / (2 alpha) is a difference of two numbers of size ~ 4.  Measured beside
them (the same elements, max over the array), the host build of the header: the same figures to two digits for gamma (ratio
0.98 - 1.00), 2.3e-15 / 8.9e-16 for empirical.  The device's figures stand in test_gpu_sindex.py and DESIGN 4.18."""
import functools
import os

import numpy as np

import sindex_np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SCALES = (1, 3, 12, 24)
DISTS = ('gamma', 'empirical')
INPUTS = (360, 72)
MAX_SHAPE = 1000.0
FACTOR = 8.0

# max |restatement - golden| over all non-NaN elements, rounded up to three digits
MEASURED = {
    (360, 'gamma', 1): 1.83e-12, (360, 'gamma', 3): 3.65e-12, (360, 'gamma', 12): 5.25e-13, (360, 'gamma', 24): 1.15e-12,
    (72, 'gamma', 1): 1.75e-12, (72, 'gamma', 3): 1.61e-12, (72, 'gamma', 12): 1.01e-12, (72, 'gamma', 24): 1.80e-12,
    (360, 'empirical', 1): 2.01e-15, (360, 'empirical', 3): 2.01e-15, (360, 'empirical', 12): 2.01e-15,
    (360, 'empirical', 24): 2.01e-15,
    (72, 'empirical', 1): 6.67e-16, (72, 'empirical', 3): 6.67e-16, (72, 'empirical', 12): 6.67e-16,
    (72, 'empirical', 24): 2.23e-16,
}


def bound(n, dist, k):
    return FACTOR * MEASURED[(n, dist, k)]


@functools.lru_cache(maxsize=None)
def _files():
    return (np.load(os.path.join(GOLDEN, 'sindex.npz'), allow_pickle=False),
            np.load(os.path.join(GOLDEN, 'sindex_72.npz'), allow_pickle=False))


def inputs(n):
    """(x [70, n], ref_month0, ref_nyear) of the golden input with n months."""
    big = _files()[0]
    ref = big['ref{}'.format(n)]
    assert tuple(big['scales']) == SCALES
    return big['x{}'.format(n)], int(ref[0]), int(ref[1])


def gold(n, dist, k):
    f = _files()[0 if n == 360 else 1]
    return f['{}_{}_{}'.format(dist, n, k)]


@functools.lru_cache(maxsize=None)
def restated(n, dist, k):
    """(index, parameters or None) of the restatement; computed once per process, never modified."""
    x, ref0, nyr = inputs(n)
    idx, par = sindex_np.std_index(x, k, ref0, nyr, dist, MAX_SHAPE)
    idx.setflags(write=False)
    if par is not None:
        par.setflags(write=False)
    return idx, par


def check_against_gold(got, n, dist, k, limit, who):
    """NaN mask identical, every clipped value exactly +-3.09, every element within ``limit`` of the golden; returns the
    largest error.  No element is left out."""
    g = gold(n, dist, k)
    got = np.asarray(got)
    assert got.shape == g.shape
    assert np.array_equal(np.isnan(got), np.isnan(g)), '{} {} {} {}: NaN masks differ at {}'.format(
        who, n, dist, k, np.argwhere(np.isnan(got) != np.isnan(g))[:5].tolist())
    m = ~np.isnan(g)
    assert np.abs(got[m]).max() <= sindex_np.CLIP
    clipped = m & (np.abs(g) == sindex_np.CLIP)
    assert np.array_equal(got[clipped], g[clipped]), '{} {} {} {}: a clipped value is not exactly +-3.09'.format(who, n, dist, k)
    err = np.where(m, np.abs(got - np.where(m, g, 0.0)), 0.0)
    c, t = np.unravel_index(err.argmax(), err.shape)
    worst = float(err[c, t])
    print('{:12s} n={:3d} {:9s} k={:2d}: max |error| {:.3g} at element ({}, {}), bound {:.3g}'.format(
        who, n, dist, k, worst, c, t, limit))
    assert worst <= limit, '{} {} {} {}: {:.3g} at element ({}, {}) exceeds {:.3g}'.format(who, n, dist, k, worst, c, t, limit)
    return worst
