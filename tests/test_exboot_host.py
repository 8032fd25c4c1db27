"""Bootstrap intervals of the GEV shape and the return levels, everything a machine without a GPU can check: the
numpy restatement (tests/exboot_np.py) against the host build of csrc/xh_exboot_dev.h (tests/exboot_probe), a replicate
against the shipped definition of xh_extremes on the explicitly resampled series, the selection against np.quantile, both
against 40-digit values, the count walk, the weights and the selection against std::sort under the sanitizers, the section's
keys and the C-ABI bookkeeping.

What is bit for bit and what is bounded.  The draws are integer arithmetic; a replicate's l1, l2, t3, t4 are +, -, x, / in a
fixed order over the sorted sample; the bounds are two order statistics and numpy's lerp: the restatement, the host build and
the device give the same bits of the draws, of the sums and of nb, and the same bits of the bounds from the same replicate
values.  k* and the levels pass through expm1, log and Gamma, which every build takes from another library:
tests/golden/make_golden_exboot.py measures how far the restatement lies from 40-digit values at 5, 10, 50 and 129 years, B =
128, in the measures of tests/exboot_cases.py, per class:

    quantity          ordinary     shifted by 1e6    steep (t3 > 0.99)    flat (t3 < -0.99)
    replicate k       2.508e-12    1.453e-08         5.708e-15            1.687e-12
    replicate level   6.120e-13    9.841e-13         4.348e-13            2.312e-16
    bound of k        3.259e-13    4.164e-09         2.006e-15            4.860e-13
    bound of a level  7.382e-14    1.714e-13         1.033e-13            5.695e-15

The bound on every implementation is 4 x the figure of its quantity and class and not below 4 ulp (the rule of DESIGN 4.21).
The steep replicates -- 1 in 500 at 5 years -- have a class of their own: within 0.01 of k = -1, Gamma(1 + k) magnifies the
rounding of k a hundred times, and the ordinary class is not loosened for them.  So have the flat ones, which resampling
makes common at few years: one low value under equal ones has t3 = -1 in exact arithmetic (96 of the golden file's
replicates), f(k) = 1 has no root, and the definition's k is the tenth Newton iterate on the float64 t3 that every build
shares, near 18.  The golden file evaluates exactly those ten steps on that t3 at 60 digits for every flat replicate, so
their figure is measured like the others.  Their levels have converged to the sample's upper end: 1 ulp."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import exboot_cases as xc
import exboot_np
import extremes_cases as cases
import extremes_np
from test_extremes_host import KINDS_LINE, edited, refused, tree, within  # noqa: F401  (tree: the fixture)
from xanthos_amd import ConfigReader, _hip

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PROBE_DIR = os.path.join(ROOT, 'tests', 'exboot_probe')
P = ctypes.c_void_p
EPS = cases.EPS
T = cases.GOLDEN_T
MEASURED = {('rep', 'k', 'ordinary'): 2.508e-12, ('rep', 'k', 'shifted'): 1.453e-08, ('rep', 'k', 'steep'): 5.708e-15,
            ('rep', 'k', 'flat'): 1.687e-12, ('rep', 'level', 'ordinary'): 6.120e-13, ('rep', 'level', 'shifted'): 9.841e-13,
            ('rep', 'level', 'steep'): 4.348e-13, ('rep', 'level', 'flat'): 2.312e-16, ('ci', 'k', 'ordinary'): 3.259e-13,
            ('ci', 'k', 'shifted'): 4.164e-09, ('ci', 'k', 'steep'): 2.006e-15, ('ci', 'k', 'flat'): 4.860e-13,
            ('ci', 'level', 'ordinary'): 7.382e-14, ('ci', 'level', 'shifted'): 1.714e-13, ('ci', 'level', 'steep'): 1.033e-13,
            ('ci', 'level', 'flat'): 5.695e-15}


def bound(golden, what, quantity, cls):
    measured = float(golden('exboot')['np_err_{}_{}_{}'.format(what, quantity, cls)])
    assert measured == pytest.approx(MEASURED[(what, quantity, cls)], rel=1e-3, abs=1e-30)        # the figure of the docstring
    return max(4.0 * measured, 4.0 * EPS)


@pytest.fixture(scope='module')
def bprobe():
    """tests/exboot_probe/libexboot_probe.so and boot_check (build() makes them; made here when the suite runs without it)."""
    path = os.path.join(PROBE_DIR, 'libexboot_probe.so')
    if not os.path.isfile(path) or not os.path.isfile(os.path.join(PROBE_DIR, 'boot_check')):
        subprocess.run(['make', '-C', PROBE_DIR], check=True, capture_output=True)
    lib = ctypes.CDLL(path)
    lib.ep_exboot.restype = ctypes.c_int
    lib.ep_exboot.argtypes = [ctypes.c_int64] + [ctypes.c_int32] * 6 + [P, ctypes.c_int32, ctypes.c_double, ctypes.c_uint64,
                                                                       ctypes.c_int64, P, P, P]
    lib.ep_draws.restype = None
    lib.ep_draws.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, P]
    lib.ep_percentile.restype = ctypes.c_double
    lib.ep_percentile.argtypes = [ctypes.c_int32, P, ctypes.c_double]
    return lib


def host_exboot(bprobe, rows, kind, B, periods=T, confidence=xc.CONFIDENCE, seed=xc.SEED, row0=0, min_years=cases.MIN_YEARS, start=0,
                nyear=None, rep=True, fill=-777.0):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    nyear = (rows.shape[1] - start) // 12 if nyear is None else nyear
    periods = np.ascontiguousarray(periods, dtype=np.float64)
    ci = np.full((rows.shape[0], 3 + 2 * periods.size), fill)
    reps = np.full((rows.shape[0], B, 5 + periods.size), fill)
    rc = bprobe.ep_exboot(rows.shape[0], rows.shape[1], start, nyear, extremes_np.KINDS.index(kind), min_years, periods.size,
                          periods.ctypes.data_as(P), B, confidence, seed, row0, rows.ctypes.data_as(P), ci.ctypes.data_as(P),
                          reps.ctypes.data_as(P) if rep else None)
    assert rc == 0
    return ci, reps


def ci_classes(ci_ref, shifted):
    """The class of every row's bounds: shifted | steep (the lower bound of k below k(t3 = 0.99)) | flat (the upper bound above
    k(t3 = -0.99)) | ordinary."""
    k_steep, k_flat = (float(extremes_np.k_of_t3(np.float64(t))) for t in (xc.STEEP_T3, -xc.STEEP_T3))
    with np.errstate(invalid='ignore'):
        return np.array(['shifted' if shifted[r] else 'steep' if ci_ref[r, 1] < k_steep else 'flat' if ci_ref[r, 2] > k_flat
                         else 'ordinary' for r in range(ci_ref.shape[0])])


def rep_classes(rep_ref, shifted):
    with np.errstate(invalid='ignore'):
        steep, flat = rep_ref[:, :, 2] > xc.STEEP_T3, rep_ref[:, :, 2] < -xc.STEEP_T3
    return np.where(np.asarray(shifted)[:, None], 'shifted', np.where(steep, 'steep', np.where(flat, 'flat', 'ordinary')))


def held(golden, got, ref, table, nbase, tag):
    """(ci, rep) against the reference's: identical NaN masks and nb, the bits of every replicate's sums, and k*, the levels and
    every bound inside the bound of their class.  ``nbase``: the rows are those of exboot_cases.make_rows(., nbase); or, as an
    array, which rows are moved by 1e6."""
    assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0])) and np.array_equal(got[0][:, 0], ref[0][:, 0]), tag
    shifted = nbase if np.ndim(nbase) else np.array([xc.row_class(r, nbase) == 'shifted' for r in range(ref[0].shape[0])])
    checks = [('ci', xc.ci_errors(got[0], ref[0], table), ci_classes(ref[0], shifted))]
    if got[1] is not None:
        assert xc.same_bits(got[1][:, :, :4], ref[1][:, :, :4]), tag
        assert np.array_equal(np.isnan(got[1]), np.isnan(ref[1])), tag
        checks.append(('rep', xc.rep_errors(got[1], ref[1]), rep_classes(ref[1], shifted)))
    for what, err, cls in checks:
        for q in xc.QUANTITIES:
            for c in xc.CLASSES:
                at = (cls == c) & ~np.isnan(err[q])
                e, b = err[q][at], bound(golden, what, q, c)
                worst = float(e.max()) if e.size else 0.0
                print('{}: {} {} ({}) max error {:.3e}, bound {:.3e}'.format(tag, what, q, c, worst, b))
                assert worst <= b, (tag, what, q, c, worst, b)


@pytest.fixture(scope='module')
def reference():
    """The restatement of the golden rows of every golden year count and kind, computed once: (ci, rep, table)."""
    out = {}
    for ny in xc.GOLDEN_YEARS:
        rows = xc.golden_rows(ny)
        for kind in extremes_np.KINDS:
            ci, rep = exboot_np.bootstrap_rows(rows, kind, T, xc.GOLDEN_B, xc.CONFIDENCE, xc.SEED, min_years=cases.MIN_YEARS)
            out[(ny, kind)] = ci, rep, extremes_np.extremes_rows(rows, kind, (), min_years=cases.MIN_YEARS)[0]
    return out


# ------------------------------------------------------------------ (1) the draws
def test_draws_of_the_restatement_are_the_host_builds(bprobe):
    for seed in (0, 1, xc.SEED, 2 ** 63 + 5, 2 ** 64 - 1):
        for n in (1, 5, 50, 255, 256, 257, 341):
            rows = np.array([0, 1, 2, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 40 + 3], dtype=np.int64)
            reps = np.array([0, 1, 63, 64, 1000, 2046, 2047])
            mine = exboot_np.draws(seed, rows, reps, n)
            assert mine.shape == (rows.size, reps.size, n) and mine.min() >= 0 and mine.max() < n
            for i, row in enumerate(rows):
                for j, b in enumerate(reps):
                    theirs = np.full(n, -1, dtype=np.int32)
                    bprobe.ep_draws(seed, int(row), int(b), n, theirs.ctypes.data_as(P))
                    assert np.array_equal(mine[i, j], theirs), (seed, n, row, b)
    # a million draws at 50 years: no cell's frequency off by more than 5 sigma
    j = exboot_np.draws(xc.SEED, np.arange(10), np.arange(2000), 50)
    freq = np.bincount(j.ravel(), minlength=50)
    sigma = np.sqrt(j.size * (1.0 / 50.0) * (1.0 - 1.0 / 50.0))
    assert j.size == 10 ** 6 and np.abs(freq - j.size / 50.0).max() <= 5.0 * sigma, np.abs(freq - j.size / 50.0).max() / sigma
    # another row, another replicate, another seed: other draws
    a = exboot_np.draws(1, [0, 1], [0, 1], 50)
    assert not np.array_equal(a[0, 0], a[0, 1]) and not np.array_equal(a[0, 0], a[1, 0])
    assert not np.array_equal(a, exboot_np.draws(2, [0, 1], [0, 1], 50))


# ------------------------------------------------------------------ (2) the replicates
@pytest.mark.parametrize('kind', extremes_np.KINDS)
@pytest.mark.parametrize('years', xc.GOLDEN_YEARS)
def test_host_build_against_the_restatement(bprobe, reference, golden, years, kind):
    got = host_exboot(bprobe, xc.golden_rows(years), kind, xc.GOLDEN_B)
    ci, rep, table = reference[(years, kind)]
    held(golden, got, (ci, rep), table, xc.GOLDEN_ROWS, 'host {} {}'.format(years, kind))
    # the bounds are numpy's quantile of the host build's own replicate values, bit for bit
    for r in np.flatnonzero(~np.isnan(got[0][:, 1])):
        assert xc.same_bits(got[0][r], exboot_np.intervals(got[1][r], xc.GOLDEN_B, xc.CONFIDENCE, kind)), (years, kind, r)


@pytest.mark.parametrize('kind', extremes_np.KINDS)
@pytest.mark.parametrize('years', xc.GOLDEN_YEARS)
def test_a_replicate_is_the_shipped_definition_on_the_resampled_series(bprobe, golden, years, kind):
    """The resampled series built explicitly, twelve equal months a year, through extremes_np.extremes_rows: n, l1, l2, t3, t4
    the same bits, k and the levels within the bounds of tests/test_extremes_host.within."""
    rows = xc.golden_rows(years)
    ci, rep = host_exboot(bprobe, rows, kind, 24)
    annual = extremes_np.annual_series(rows, kind)
    zs = np.sort(-annual if kind == 'min' else annual, axis=1, kind='stable')
    checked = 0
    for r in np.flatnonzero(ci[:, 0] > 0):
        n = int((~np.isnan(zs[r])).sum())
        j = exboot_np.draws(xc.SEED, [r], np.arange(24), n)[0]                       # [24, n]
        series = np.repeat(zs[r][j], 12, axis=1)                                      # twelve equal months per year
        ref = extremes_np.extremes_rows(series, 'max', T, min_years=cases.MIN_YEARS)
        fit = ~np.isnan(ref[0][:, 5])
        assert np.array_equal(fit, ~np.isnan(rep[r, :, 4])) and (ref[0][:, 0] == n).all()
        lm = extremes_np.lmoments(np.sort(zs[r][j], axis=1))                         # (the sums of a replicate without a fit)
        assert xc.same_bits(rep[r, :, :4], np.stack(lm[1:5], axis=1)), (years, kind, r)
        assert xc.same_bits(rep[r, fit, :4], ref[0][fit, 1:5]), (years, kind, r)
        got_table = np.concatenate([ref[0][:, :1], rep[r, :, :5], ref[0][:, 6:8], rep[r, :, 5:]], axis=1)
        got_table[~fit, 3:5] = np.nan
        within(golden, (got_table, ref[1], ref[2]), ref, 'resampled {} {} row {}'.format(years, kind, r), quantities=('k', 'level'),
               classes=xc.row_class(r, xc.GOLDEN_ROWS))
        checked += int(fit.sum())
    assert checked > 200


# ------------------------------------------------------------------ (3) the selection
def test_selection_and_lerp_are_numpys_linear_quantile(bprobe):
    rng = np.random.default_rng(11)
    for nb in (2, 3, 64, 65, 1000, 2048):
        for trial in range(3):
            v = np.concatenate([rng.normal(0.0, 30.0, nb), rng.integers(-5, 5, nb) / 3.0])[rng.permutation(2 * nb)[:nb]]
            v = np.ascontiguousarray(np.where(v == 0.0, 0.25, v))
            seen = set()
            for p in (0.05, 0.95, 0.025, 0.975, 0.5, 0.3, 0.77, 0.001, 0.999, 1.0 / 3.0, 0.45):
                h = (nb - 1) * p
                seen.add(h - np.floor(h) < 0.5)
                got = bprobe.ep_percentile(nb, v.ctypes.data_as(P), p)
                want = np.quantile(v, p, method='linear')
                assert got == want and np.float64(got).tobytes() == np.float64(want).tobytes(), (nb, p, got, want)
            assert seen == {True, False} or nb == 2


# ------------------------------------------------------------------ (4) 40 digits
@pytest.mark.parametrize('kind', extremes_np.KINDS)
@pytest.mark.parametrize('years', xc.GOLDEN_YEARS)
def test_restatement_and_host_build_against_40_digits(bprobe, reference, golden, years, kind):
    g_ci = golden('exboot')['ci_{}_{}'.format(kind, years)]
    ci, rep, table = reference[(years, kind)]
    assert g_ci.shape == (xc.GOLDEN_ROWS + xc.GOLDEN_SPARSE, 3 + 2 * len(T))
    held(golden, (ci, None), (g_ci, None), table, xc.GOLDEN_ROWS, 'restatement {} {}'.format(years, kind))
    held(golden, (host_exboot(bprobe, xc.golden_rows(years), kind, xc.GOLDEN_B)[0], None), (g_ci, None), table, xc.GOLDEN_ROWS,
         'host {} {}'.format(years, kind))


# ------------------------------------------------------------------ (5) masks and the halving rule
@pytest.mark.parametrize('years', xc.GOLDEN_YEARS)
def test_masks_and_the_halving_rule(bprobe, years):
    """The 300 rows of the device test and the sparse rows, through the host build (whose nb is the restatement's, bit for bit:
    test_host_build_against_the_restatement; the sparse rows are put through the restatement here as well)."""
    nbase = 300
    rows = xc.make_rows(years, nbase)
    kinds = np.array([cases.kind_of(r) for r in range(nbase)])
    for kind in extremes_np.KINDS:
        table = extremes_np.extremes_rows(rows, kind, (), min_years=cases.MIN_YEARS)[0]
        fit = ~np.isnan(table[:, 5])
        ci = host_exboot(bprobe, rows, kind, xc.GOLDEN_B, rep=False)[0]
        assert ((ci[:, 0] > 0) == fit).all() and np.isnan(ci[~fit, 1:]).all() and (ci[~fit, 0] == 0).all()
        have = ~np.isnan(ci[:, 1])
        assert np.array_equal(have, 2 * ci[:, 0] >= xc.GOLDEN_B) and np.array_equal(np.isnan(ci[:, 1:]).all(axis=1), ~have)
        assert np.array_equal(np.isnan(ci[:, 1:]).any(axis=1), ~have)
        # test_gpu_extremes' own condition on fits, on intervals
        assert have[:nbase].sum() > nbase // 3 and (~have[:nbase]).sum() > nbase // 10 and (~fit[:nbase]).sum() >= 60
        # no row of make_rows comes near nb < B / 2 but the two-valued ones (ties, signed_zeros: a 'two' row by another name)
        low = np.flatnonzero(fit[:nbase] & (ci[:nbase, 0] < 0.8 * xc.GOLDEN_B))
        assert set(kinds[low]) <= {'ties', 'signed_zeros'}, (years, kind, kinds[low])
        assert (ci[:nbase][have[:nbase], 1] <= ci[:nbase][have[:nbase], 2]).all()
        lo, hi = (ci[:, 3::2], ci[:, 4::2])
        assert (lo[have] <= hi[have]).all()
    # the sparse rows at the B of the device test's shapes: 'one' never fits, 'six' always has intervals, 'two' has about 0.6 B
    sparse = xc.sparse_rows(years)
    two, one, six = slice(0, xc.TWO_ROWS), slice(xc.TWO_ROWS, xc.TWO_ROWS + xc.ONE_ROWS), slice(xc.TWO_ROWS + xc.ONE_ROWS, None)
    under = {}
    for B in (2, 64, 65, 1000):
        ci = host_exboot(bprobe, sparse, 'max', B, rep=False, row0=nbase)[0]
        if B <= 65:
            ref = exboot_np.bootstrap_rows(sparse, 'max', T, B, xc.CONFIDENCE, xc.SEED, row0=nbase, min_years=cases.MIN_YEARS)[0]
            assert np.array_equal(ci[:, 0], ref[:, 0]) and np.array_equal(np.isnan(ci), np.isnan(ref))
        assert (ci[one, 0] == 0).all() and np.isnan(ci[one, 1:]).all()
        assert (ci[six, 0] >= (0.75 * B if B > 2 else 1)).all() and not np.isnan(ci[six, 1:]).any()
        assert (ci[two, 0] <= B).all() and np.array_equal(np.isnan(ci[two, 1]), 2 * ci[two, 0] < B)
        under[B] = int(np.isnan(ci[two, 1]).sum())
        if B == 1000:
            assert under[B] == 0 and (np.abs(ci[two, 0] / B - (0.663 if years == 5 else 0.60)) < 0.06).all()
    # the halving rule is exercised: at B = 2, and at 64 or 65, some of the 40 'two' rows are under half and most are not
    print(years, 'two-rows under half:', under)
    # (at 5 years a replicate fits with P = 0.663 and nb < 32 of 64 is one row in 300: B = 2 alone reaches the rule there)
    assert 1 <= under[2] <= 20 and (under[64] + under[65] >= 1 or years == 5) and under[64] <= 12 and under[65] <= 12


# ------------------------------------------------------------------ (6) min is max of the negated rows
@pytest.mark.parametrize('years', xc.GOLDEN_YEARS)
def test_min_is_max_of_the_negated_rows_bit_for_bit(bprobe, years):
    rows = xc.golden_rows(years)
    for f in (lambda r, kind: host_exboot(bprobe, r, kind, 64),
              lambda r, kind: exboot_np.bootstrap_rows(r, kind, T, 64, xc.CONFIDENCE, xc.SEED, min_years=cases.MIN_YEARS)):
        (lo_ci, lo_rep), (hi_ci, hi_rep) = f(rows, 'min'), f(-rows, 'max')
        assert xc.same_bits(lo_rep, hi_rep) and xc.same_bits(lo_ci[:, :3], hi_ci[:, :3])
        assert xc.same_bits(lo_ci[:, 3::2], -hi_ci[:, 4::2]) and xc.same_bits(lo_ci[:, 4::2], -hi_ci[:, 3::2])
        assert (~np.isnan(lo_ci[:, 1])).any()


# ------------------------------------------------------------------ (7) counter-based
def test_prefix_of_replicates_slices_of_rows_and_seeds(bprobe):
    rows = xc.golden_rows(50)
    for f in (lambda r, B, **kw: host_exboot(bprobe, r, 'max', B, **kw),
              lambda r, B, seed=xc.SEED, row0=0: exboot_np.bootstrap_rows(r, 'max', T, B, xc.CONFIDENCE, seed, row0=row0,
                                                                            min_years=cases.MIN_YEARS)):
        small, large = f(rows, 64), f(rows, 130)
        assert xc.same_bits(small[1], large[1][:, :64]) and not xc.same_bits(small[0], large[0])
        part = f(rows[7:19], 64, row0=7)
        assert xc.same_bits(part[0], small[0][7:19]) and xc.same_bits(part[1], small[1][7:19])
        assert not xc.same_bits(f(rows[7:19], 64)[1], small[1][7:19])
        other = f(rows, 64, seed=xc.SEED + 1)
        assert not xc.same_bits(other[1], small[1]) and np.array_equal(np.isnan(other[0][:, 1]), np.isnan(small[0][:, 1]))


def test_probe_refuses_what_the_entry_refuses(bprobe):
    x = np.zeros((2, 130))
    periods = np.array([2.0, 10.0])
    ci, rep = np.full((2, 7), -777.0), np.full((2, 8, 7), -777.0)

    def call(stride=130, col0=0, nyear=10, kind=0, min_years=5, nT=2, periods=periods, B=8, confidence=0.9, row0=0, x=x, ci=ci):
        return bprobe.ep_exboot(2, stride, col0, nyear, kind, min_years, nT, None if periods is None else periods.ctypes.data_as(P), B,
                                confidence, 1, row0, None if x is None else x.ctypes.data_as(P), None if ci is None else ci.ctypes.data_as(P),
                                rep.ctypes.data_as(P))
    for bad in (dict(x=None), dict(ci=None), dict(periods=None), dict(col0=-1), dict(col0=11), dict(nyear=0), dict(stride=5000, nyear=342),
                dict(nT=9), dict(periods=np.array([2.0, 1.0])), dict(kind=2), dict(min_years=4), dict(B=1), dict(B=2049), dict(B=0),
                dict(confidence=0.0), dict(confidence=1.0), dict(confidence=float('nan')), dict(row0=-1)):
        assert call(**bad) == 1, bad
    assert (ci == -777.0).all() and (rep == -777.0).all()
    assert call() == 0 and call(B=2) == 0 and call(nT=0, periods=None) == 0


# ------------------------------------------------------------------ (8) under the sanitizers
def test_count_walk_weights_and_selection_under_sanitizers(bprobe):
    """xh_exb_count, xh_exb_fit, xh_exb_weight, xh_exb_sort_stage, xh_exb_percentile and xh_exboot_row in a stand-alone program of
    their own (tests/exboot_probe/boot_check.cpp, -fsanitize=address,undefined), started as a child process: rows with ties,
    signed zeros and missing years at 1 .. 8, 63, 64, 65, 128, 129, 255, 256, 257 and 341 years and random counts (the count is 16
    bits wide at every one of them: there is no layout switch), teams of 1, 3 and 64 lanes (the kernel's width), in buffers of
    exactly the kernel's sizes, against std::sort of the explicit resample."""
    out = subprocess.run([os.path.join(PROBE_DIR, 'boot_check'), '90', '20263'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and re.search(r'90 cases, \d+ with a fit, 0 failed', out.stdout), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(re.search(r'(\d+) with a fit', out.stdout).group(1)) > 45


# ------------------------------------------------------------------ (9) the section
def test_section_keys_and_their_defaults(tree, tmp_path):  # noqa: F811
    root, w, f, plain, ini = tree
    base = ConfigReader(ini)
    assert base.extremes_bootstrap is None and ConfigReader(plain).extremes_bootstrap is None
    c = ConfigReader(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, min\nbootstrap = 500')))
    assert c.extremes_bootstrap == {'B': 500, 'confidence': 0.90, 'seed': 1}
    assert c.extremes == base.extremes and 'bootstrap' not in c.extremes and 'confidence' not in c.extremes
    c = ConfigReader(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, min\nbootstrap = 2048\nconfidence = 0.5\nbootstrap_seed = 18446744073709551615')))
    assert c.extremes_bootstrap == {'B': 2048, 'confidence': 0.5, 'seed': 2 ** 64 - 1} and c.extremes == base.extremes
    assert ConfigReader(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, min\nbootstrap = 100\nbootstrap_seed = 0'))).extremes_bootstrap['seed'] == 0
    zero = ConfigReader(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, min\nbootstrap = 0')))
    assert zero.extremes_bootstrap is None and zero.extremes == base.extremes


def test_refusals_of_the_bootstrap_keys_name_their_key(tree, tmp_path):  # noqa: F811
    root, w, f, plain, ini = tree
    for bad in ('99', '2049', '-5', 'many', '100.5', '1e3'):
        refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nbootstrap = ' + bad)), 'bootstrap', bad)
    for bad in ('0', '1', '1.5', '-0.9', 'high', 'nan'):
        refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nbootstrap = 200\nconfidence = ' + bad)), 'confidence', bad)
    for bad in ('-1', '1.5', 'seed', '18446744073709551616'):
        refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nbootstrap = 200\nbootstrap_seed = ' + bad)), 'bootstrap_seed', bad)
    # the two that belong to the intervals, without them
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nconfidence = 0.9')), 'confidence', 'bootstrap')
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nbootstrap_seed = 3')), 'bootstrap_seed', 'bootstrap')
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nbootstrap = 0\nconfidence = 0.9')), 'confidence', 'bootstrap')
    # a handed-in fit has no sample of this run to resample
    stem = os.path.join(str(tmp_path), 'historic', 'hist')
    os.makedirs(os.path.dirname(stem))
    for var in ('q', 'avgchflow'):
        np.save(os.path.join(str(tmp_path), 'historic', 'extremes_{}_max_hist.npy'.format(var)), np.zeros((w.ncell, 14)))
    assert ConfigReader(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nparameters = ' + stem))).extremes_bootstrap is None
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nbootstrap = 200\nparameters = ' + stem)), 'bootstrap', 'parameters')


# ------------------------------------------------------------------ the C-ABI entry
def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    assert re.search(r'\bint xh_extremes_boot\(xh_ctx \*ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t kind, '
                     r'int32_t min_years,\s+int32_t nT, const double \*h_T, int32_t B, double confidence, uint64_t seed, int64_t row0, '
                     r'const double \*d_x,\s+double \*d_ci, double \*d_rep\);', header)
    assert re.search(r'#define XH_EXB_MAX_B 2048\b', header) and 'xh_extremes_boot replaces NO function of the reference' in header
    assert len(_hip.SIGNATURES['xh_extremes_boot'][1]) == 16 and len(_hip.SIGNATURES['xh_extremes'][1]) == 14
    assert hasattr(_hip.lib(), 'xh_extremes_boot') and _hip.lib().xh_abi_version() == _hip.ABI_VERSION == 7
    assert hasattr(_hip.Context, 'extremes_boot')
    from xanthos_amd import extremes
    assert extremes.CI_COLUMNS == ('nb', 'k_lo', 'k_hi') and callable(extremes.bootstrap_rows)
    dev = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'xh_exboot_dev.h')).read()
    assert re.search(r'#define XH_EXB_MAX_B {}\b'.format(exboot_np.MAX_B), dev) and '#include "xh_extremes_dev.h"' in dev
    assert re.search(r'#define XH_EXB_NREP {}\b'.format(exboot_np.NREP), dev)
    # the library's splitmix64, restated: the constants of csrc/xh_calib_de.hip
    for name in ('xh_calib_de.hip', 'xh_exboot_dev.h'):
        text = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', name)).read()
        assert all(c in text for c in ('0x9E3779B97F4A7C15ull', '0xBF58476D1CE4E5B9ull', '0x94D049BB133111EBull', '0xD1342543DE82EF95ull'))
