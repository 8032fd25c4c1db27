"""The rows, shapes and error measures of the bootstrap tests, shared by tests/test_exboot_host.py,
tests/test_gpu_exboot.py and tests/golden/make_golden_exboot.py.

The rows are those of tests/extremes_cases.make_rows followed by SPARSE rows, all zero but a few positive years:
  'one'   one positive year: t3 = 1, the row itself has no fit;
  'two'   two different positive years: the sparsest row that has a fit.  A replicate of it has a fit when it draws the
          positive years at least twice (one draw: its only non-zero year is its largest, t3 = 1; none: constant), which at n
          years is P(Binomial(n, 2 / n) >= 2): 0.663 at 5 years, 0.594 = 1 - 3 e^-2 in the limit.  (About 40 % is the share
          WITHOUT a fit.)  So no row with a fit expects nb < B / 2, and the halving rule is reached by chance only: at B = 2
          (nb = 0, one such row in six or nine) and, among TWO_ROWS = 40 such rows, at B = 64 or 65 (nb < 32: one row in 15
          to 40);
  'six'   six positive years (four at 5 years): well above half, P = 0.98.
With 128 replicates the rows of make_rows themselves go down to nb = 0.516 B (two signed_zeros rows at 50 years, min, whose
negated minima are 48 zeros and two ones: the 'two' row again)."""
import numpy as np

import extremes_cases as cases

TWO_ROWS, ONE_ROWS, SIX_ROWS = 40, 4, 4
SPARSE_ROWS = TWO_ROWS + ONE_ROWS + SIX_ROWS
GOLDEN_YEARS = (5, 10, 50, 129)
GOLDEN_B = 128
GOLDEN_ROWS = cases.HOST_ROWS                    # the host rows of extremes_cases ...
GOLDEN_SPARSE = 6                                # ... and the sparse rows 0, 8, 16, .. 40: five 'two', one 'one'
CONFIDENCE = 0.90
SEED = 20264
# the device shapes: every year count of the wave boundary and the ends, B on both sides of 64 (one round of the wavefront), of
# the powers of two the sort pads to, and the ends of the range -- spread over the year counts, not the full product.  (341 years
# with B = 1000 is the one shape here whose workgroup asks for more than 64 KB of LDS; with 2048 the host build alone would take
# five seconds.)
DEVICE_SHAPES = ((5, 2), (5, 1000), (10, 2048), (63, 65), (64, 257), (65, 2048), (129, 1000), (341, 64), (341, 1000))
GRID_CAP = 8 * 256                               # the most workgroups xh_extremes_boot launches: beyond it a workgroup walks several rows
QUANTITIES = ('k', 'level')
CLASSES = ('ordinary', 'shifted', 'steep', 'flat')
STEEP_T3 = 0.99                                  # steep: a replicate with t3 above it, k < -0.985, where Gamma(1 + k) magnifies;
#                                                  flat: t3 below -0.99, k > 7.6, where f(k) - 1 = 2^-k; towards t3 = -1 the
#                                                  definition's k is the tenth Newton iterate, near 18, not a root


def t3_class(t3):
    return 'steep' if t3 > STEEP_T3 else 'flat' if t3 < -STEEP_T3 else 'ordinary'


def sparse_rows(nyear, seed=0):
    rng = np.random.default_rng(7000 + 10 * nyear + seed)
    rows = np.zeros((SPARSE_ROWS, 12 * nyear))
    for r in range(SPARSE_ROWS):
        m = 2 if r < TWO_ROWS else 1 if r < TWO_ROWS + ONE_ROWS else min(6, nyear - 1)
        years = rng.choice(nyear, m, replace=False)
        rows[r, 12 * years + rng.integers(0, 12, m)] = np.sort(rng.uniform(1.0, 60.0, m)) + np.arange(m)
    return rows


def make_rows(nyear, nrows, seed=0):
    """``nrows`` rows of extremes_cases.make_rows, then the SPARSE_ROWS sparse ones."""
    return np.concatenate([cases.make_rows(nyear, nrows, seed), sparse_rows(nyear, seed)], axis=0)


def golden_rows(nyear):
    return np.concatenate([cases.make_rows(nyear, GOLDEN_ROWS), sparse_rows(nyear)[::8][:GOLDEN_SPARSE]], axis=0)


def row_class(r, nbase):
    """Of row r of make_rows(., nbase): the sparse rows are ordinary."""
    return cases.class_of(r) if r < nbase else 'ordinary'


def rep_errors(rep, ref):
    """rep, ref [..., 5 + nT] -> {'k', 'level': [...]} in the measures of extremes_cases.errors, NaN without a fit: k against
    max(|k|, K_FLOOR), a level against the largest of |level|, |l1*| and l2* of the reference's replicate."""
    with np.errstate(invalid='ignore', divide='ignore'):
        k = np.abs(rep[..., 4] - ref[..., 4]) / np.maximum(np.abs(ref[..., 4]), cases.K_FLOOR)
        scale = np.maximum(np.abs(ref[..., 0]), ref[..., 1])[..., None]
        lev = np.abs(rep[..., 5:] - ref[..., 5:]) / np.maximum(np.abs(ref[..., 5:]), scale)
        level = lev.max(axis=-1) if lev.shape[-1] else np.where(np.isnan(k), np.nan, 0.0)
    return {'k': k, 'level': level}


def ci_errors(ci, ref, table):
    """ci, ref [nrows, 3 + 2 nT] and the rows' table (l1, l2 in columns 1, 2) -> {'k', 'level': [nrows]}, NaN without bounds: the
    bounds of k against max(|k bound|, K_FLOOR), the bounds of a level against the largest of |bound|, |l1| and l2 of the row."""
    with np.errstate(invalid='ignore', divide='ignore'):
        k = (np.abs(ci[:, 1:3] - ref[:, 1:3]) / np.maximum(np.abs(ref[:, 1:3]), cases.K_FLOOR)).max(axis=1)
        scale = np.maximum(np.abs(table[:, 1]), table[:, 2])[:, None]
        lev = np.abs(ci[:, 3:] - ref[:, 3:]) / np.maximum(np.abs(ref[:, 3:]), scale)
        level = lev.max(axis=1) if lev.shape[1] else np.where(np.isnan(k), np.nan, 0.0)
    return {'k': k, 'level': level}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.where(np.isnan(a), 0.0, a).tobytes() == np.where(
        np.isnan(b), 0.0, b).tobytes()
