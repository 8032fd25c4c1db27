"""Penman-Monteith class by class at every branch (-m gpu): csrc/xh_pm.hip against the long-double truth.

The kernel is not a transcription of the reference (reciprocal resistances, one common denominator, two tests for three
ways to rs = 1e5, exp instead of pow, fdiv), and the older tests (test_gpu_parity.py: test_pm_golden,
test_pm_synthetic_vs_oracle, test_two_leap_year_rules_on_the_device) only ever show it cells that mix eight ordinary
classes.  Here every cell holds ONE class (tests/pm_cases.py), each class carries one edge of the tables, and the forcing
walks over every step of the model; tests/test_pm_host.py asserts that every branch is reached and ties the truth
(tests/pm_np.py) to the real reference.  The bar is the project's: |got - true| <= 1e-9 |true| + 1e-9 mm.

Measured on MI355X (gfx950); the asserts hold the bar, these are the observed figures, as fractions of the bar:
  whole case set, worst per index pair .. (0, 6) 2.0e-2, (6, 0) 2.0e-2, (2, 7) 3.0e-2, (3, 3) 3.0e-2, (6, 6) 2.0e-2
  per forcing family, worst pair ........ a 8.8e-3, b 1.1e-2, c 1.3e-2, d 6.7e-3, e 2.0e-2, f 3.0e-2, z 0 (exact zeros)
  per class as vegetation ............... 0 1.6e-2, 1 6.6e-3, 2 1.5e-2, 3 2.0e-2, 4 7.8e-3, 5 1.3e-2, 6 3.0e-2, 7 7.0e-3
  a class as water or snow .............. at most 1.1e-5
  nlcs 7 / 32 ........................... 4.1e-2 / 3.0e-2;  from 1899 / 2099 / 1985 / 1986 / 2001: 2.6e-2 / 2.0e-2 / 1.3e-2 / 1.3e-2 / 2.0e-2
  worst RELATIVE error .................. 5.7e-11 where PET >= 1 mm, 5.8e-11 where PET >= 1e-3 mm -- not the 5e-13 that the
                                          kernel's head comment gave for mixed cells against numpy; the comment now says so.
                                          The double reference itself is 1.3e-2 of the bar from the same truth.
  pairs left out (on a computed threshold) 0 of 46,080 for every index pair
  every bit comparison (launch shapes, tairprev NULL, paired against plain kernel) held.

The defect these tests found: with water_idx == snow_idx the kernel took albedo row 0 (it tested the water index first
for the row, the snow index first for the formula), the reference row 6 (snow is assigned last, penman_monteith.py:460-464).
On the parent commit [pair3] and [pair4] of test_every_class_alone_at_every_branch and of
test_exact_zeros_stay_zero_and_nothing_is_nan fail (3,863 and 3,772 values beyond the bar, up to 4.8e8 of it) and
everything else here passes; with the snow test first all pass.

Mutation check (done once on scratch copies of csrc/xh_pm.hip, nothing of it kept).  "old" are the three older tests named
above (four cases); the six launch-shape tests, the paired-kernel test and the nlcs = 33 test compare the kernel with itself
(or never launch it) and pass throughout.
  mutation                                                   new tests failing                              old
  drop `rs = gsum < 0.0001 ? 0.0001 : rs`                    17: whole set x5, zeros x5, nlcs x2, calendar x5    pass
  `lai < 0.0001` -> `lai < 0.00001` in rs                     11: whole set x4 (not (3, 3)), nlcs x2, calendar x5  pass
  drop `&& rhc_raw <= rslimit` (the cap on rhc)              17, as the first                                   FAIL
  albedo row by swapped index ((6, 0): snow row 0, water 6)   2: whole set and zeros of pair (6, 0)               pass
  drop `fc = fc > 1.0 ? 1.0 : fc` (xh_pm_prepare)             17, as the first                                   pass
  `lai > 0.00001` -> `lai > 0.000001` in use_rhc              11, as the second                                  pass
Two findings.  The `lai < 0.0001` mutation ESCAPED the first version of the case set (all 25 passed): rs = 1e5 and the
quotient it replaces, never below rc / lai = 2e5, both end at rslimit <= 2000, so the branch cannot show under any ordinary
cap.  Class 3 now has rslimit = 1e6 and laimax = 2e-4 in the months of tiny lai (a canopy share to transpire through that
resistance), test_pm_host.py asserts that this combination is reached (branch `rs_1e5_seen`), and the mutation fails as
listed.  The cap on rhc is not a gap: the older inputs reach it wherever fwet is small, and their tests fail with it too; the
last two mutations were added in its place.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import pm_cases
import pm_np

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-9          # test_gpu_parity.close, smoke()


@pytest.fixture(scope='module')
def hip():
    from xanthos_amd import _hip
    assert _hip.device_count() > 0, 'no GPU visible'
    return _hip


@pytest.fixture(scope='module')
def cs():
    return pm_cases.case_set()


@pytest.fixture(scope='module')
def truth(cs):
    return pm_np.run(cs.data, cs.nlcs, cs.start_year, cs.end_year, cs.lc_years)


@pytest.fixture(scope='module')
def whole(hip, cs):
    """PET of the whole case set through the plugin entry point, once per index pair."""
    from xanthos_amd.pet import penman_monteith as pm
    cache = {}

    def get(pair):
        if pair not in cache:
            cache[pair] = pm.run_pmpet(cs.data, cs.ncell, cs.nlcs, cs.start_year, cs.end_year, pair[0], pair[1], cs.lc_years)
        return cache[pair]
    return get


def device_pet(hip, d, ncell, nlcs, y0, y1, pair, lc_years, tairprev):
    """run_pmpet_device on uploaded arrays; ``tairprev`` False passes NULL (the kernel reads the previous cell itself)."""
    from xanthos_amd.pet import penman_monteith as pm
    ctx = hip.get_context(0)
    nm = 12 * (y1 - y0 + 1)
    up = lambda a: ctx.upload(np.ascontiguousarray(np.asarray(a)[:, :nm]))
    bufs = [up(d.tair_load), up(d.TMIN_load), up(d.rhs_load), up(d.wind_load), up(d.rsds_load), up(d.rlds_load),
            up(d.tairprev_load) if tairprev else None, ctx.upload(np.ascontiguousarray(d.lct_load)),
            ctx.upload(np.ascontiguousarray(d.elev.reshape(-1)))]
    d_pet = pm.run_pmpet_device(ctx, pm.tables_from(d, nlcs), ncell, y0, y1, pair[0], pair[1], lc_years, *bufs)
    out = d_pet.download()
    for b in bufs + [d_pet]:
        if b is not None:
            b.free()
    return out


def ratio_to_bar(got, true):
    assert got.shape == true.shape and got.dtype == np.float64
    assert np.isfinite(got).all(), '{} values are NaN or infinite'.format(int((~np.isfinite(got)).sum()))
    return (np.abs(got - true) / (RTOL * np.abs(true) + ATOL)).astype(np.float64)


def held(got, true, skip, tag):
    """The bar, everywhere but at ``skip`` (pairs on a computed threshold); returns the ratios."""
    r = ratio_to_bar(got, true)
    bad = (r > 1.0) & ~skip
    if bad.any():
        at = np.unravel_index(np.argmax(np.where(skip, 0.0, r)), r.shape)
        raise AssertionError('{}: {} values beyond the bar, worst {:.3e} of it at cell {} month {}: got {!r}, true {!r}'.format(
            tag, int(bad.sum()), r[at], at[0], at[1], got[at], float(true[at])))
    return np.where(skip, 0.0, r)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ======================================================================================== the whole case set, per pair
@pytest.mark.parametrize('pair', pm_cases.INDEX_PAIRS)
def test_every_class_alone_at_every_branch(cs, truth, whole, pair):
    """The five index pairs on the whole case set; the ties (3, 3) and (6, 6) are snow with albedo row 6, as in the
    reference, where snow is assigned last (penman_monteith.py:460-464)."""
    got, true = whole(pair), truth.pet(*pair)
    skip = truth.near_threshold(*pair)
    assert skip.sum() <= 1e-3 * skip.size
    r = held(got, true, skip, 'pair {}'.format(pair))
    klass = pm_cases.class_by_month(cs)
    fam = np.broadcast_to(cs.family[:, None], r.shape)
    print('pair {}: worst {:.3e} of the bar'.format(pair, r.max()))
    print('  by family: ' + ', '.join('{} {:.2e}'.format(n, r[fam == f].max()) for f, n in enumerate(cs.family_names)))
    print('  by class:  ' + ', '.join('{} {:.2e}'.format(l, r[klass == l].max()) for l in range(cs.nlcs)))
    for floor in (1.0, 1e-3):
        m = np.abs(true) >= floor
        print('  worst relative error where PET >= {:g} mm: {:.3e}'.format(
            floor, float(np.max(np.abs(got[m] - true[m]) / np.abs(true[m])))))


@pytest.mark.parametrize('pair', pm_cases.INDEX_PAIRS)
def test_exact_zeros_stay_zero_and_nothing_is_nan(cs, truth, whole, pair):
    """Where the truth is exactly 0 -- the clamps of water, snow and eet < 0, a cell without land cover -- the device returns
    0 (of either sign), and no NaN or infinity appears anywhere (RH = 0 makes log(rh / 100) = -inf inside)."""
    got, true = whole(pair), truth.pet(*pair)
    assert np.isfinite(got).all()
    zero = true == 0
    assert zero.sum() > 1000
    assert (got[zero] == 0).all(), '{} of {} exact zeros are not zero on the device, largest {!r}'.format(
        int((got[zero] != 0).sum()), int(zero.sum()), float(np.abs(got[zero]).max()))
    assert (got >= 0).all()
    # RH < 70 (fwet = 0) and fc == 0 in vegetated classes: the canopy terms vanish and the soil term remains
    for name in ('fwet_0', 'fc_0'):
        sel = truth.taken(name, *pair).any(axis=0)
        assert sel.sum() >= 8 and (got[sel] > 0).any()


# ======================================================================================== launch shapes
@pytest.mark.parametrize('ncell', [1, 2, 63, 64, 65, 257])
def test_result_does_not_depend_on_the_launch(hip, cs, whole, ncell):
    """The first ncell cells and 12 / 24 months, with tairprev given and with NULL (the kernel then reads the previous
    cell, and 0 for cell 0): the same bits as those rows of the whole run.  One thread handles a pair of months in a
    grid-stride loop with whole passes; nothing of that may show."""
    from xanthos_amd.pet import penman_monteith as pm
    want = whole((0, 6))
    for nm in (12, 24):
        y1 = cs.start_year + nm // 12 - 1
        d = pm_cases.first_cells(cs.data, ncell, nm)
        got = pm.run_pmpet(d, ncell, cs.nlcs, cs.start_year, y1, 0, 6, cs.lc_years)
        assert same_bits(got, want[:ncell, :nm]), (ncell, nm, 'tairprev given')
        got = device_pet(hip, d, ncell, cs.nlcs, cs.start_year, y1, (0, 6), cs.lc_years, tairprev=False)
        assert same_bits(got, want[:ncell, :nm]), (ncell, nm, 'tairprev NULL')


# ======================================================================================== class counts
@pytest.mark.parametrize('nlcs', [7, 32])
def test_class_counts(hip, nlcs):
    """The least and the most classes the library takes (XH_MAX_LCS = 32), tables tiled from the edge set."""
    from xanthos_amd.pet import penman_monteith as pm
    c = pm_cases.case_set(nlcs)
    t = pm_np.run(c.data, nlcs, c.start_year, c.end_year, c.lc_years)
    got = pm.run_pmpet(c.data, c.ncell, nlcs, c.start_year, c.end_year, 0, 6, c.lc_years)
    r = held(got, t.pet(0, 6), t.near_threshold(0, 6), 'nlcs {}'.format(nlcs))
    print('nlcs {}: worst {:.3e} of the bar'.format(nlcs, r.max()))
    assert sorted(np.unique(c.klass[c.klass >= 0])) == list(range(nlcs))


def test_more_classes_than_the_library_takes(hip):
    from xanthos_amd.pet import penman_monteith as pm
    c = pm_cases.case_set(33)
    d = pm_cases.first_cells(c.data, 64, 12)
    with pytest.raises(hip.HipError, match='XH_MAX_LCS'):
        pm.run_pmpet(d, 64, 33, c.start_year, c.start_year, 0, 6, c.lc_years)


# ======================================================================================== calendar
@pytest.mark.parametrize('y0', [1899, 2099, 1985, 1986, 2001])
def test_calendar(hip, cs, y0):
    """Two years from 1899 and 2099 (1900 and 2100 are no leap years for calendar.isleap) and from 1985 / 1986 / 2001 (the
    land-cover slice: the first year with x - year >= -4, the last slice from its year on): the class a cell holds moves
    with the slice, so a wrong slice is another class's ET."""
    from xanthos_amd.pet import penman_monteith as pm
    d = pm_cases.first_cells(cs.data, cs.ncell, 24)
    t = pm_np.run(d, cs.nlcs, y0, y0 + 1, cs.lc_years)
    got = pm.run_pmpet(d, cs.ncell, cs.nlcs, y0, y0 + 1, 0, 6, cs.lc_years)
    r = held(got, t.pet(0, 6), t.near_threshold(0, 6), 'from {}'.format(y0))
    print('from {}: worst {:.3e} of the bar'.format(y0, r.max()))
    assert not t.branches['leap_february'].any()          # none of these runs has a 29-day February


# ======================================================================================== the paired kernel
def test_paired_kernel_equals_the_plain_one_in_bits(hip, cs):
    """k_pm_pet2 runs only as the filler of a fed run (xh_run_fused mode 1, months behind the first block).  On the
    4,000-cell world of test_fused_pipeline_equals_stage_by_stage, with the six PM forcings replaced by the families a, d
    and e of the case set tiled over the cells (the world keeps its own tables: ABCD and the routing see ordinary PET), PET
    of the fed order equals PET of the stage-by-stage order in bits."""
    from xanthos_amd import synth
    from xanthos_amd.pipeline import OUTPUTS, pipeline_from_world
    ctx = hip.get_context(0)
    w = synth.make_world(nrow=60, ncol=120, ncell=4000, n_basins=11, seed=8)
    nm = 120
    pipe = pipeline_from_world(ctx, w, nm, 1971, 25, 6)
    ctx.synth_forcing(17, w.ncell, nm, ctx.upload(w.latitude), pipe.alloc_forcing(), nan_frac=0.002)
    rows = np.nonzero(np.isin(cs.family, [cs.family_names.index(k) for k in 'ade']))[0]
    take, mon = rows[np.arange(w.ncell) % len(rows)], np.arange(nm) % cs.nmonths
    pipe.set_forcing({k: np.ascontiguousarray(getattr(cs.data, f)[take][:, mon]) for k, f in (
        ('tas', 'tair_load'), ('tmin', 'TMIN_load'), ('rhs', 'rhs_load'), ('wind', 'wind_load'), ('rsds', 'rsds_load'),
        ('rlds', 'rlds_load'))})
    pipe.run(fed=False, fused=False)
    ref = pipe.download()
    assert np.isfinite(ref['pet']).all() and (ref['pet'] == 0).sum() > 1000 and ref['pet'].max() > 50.0
    n0 = ctx.timing('feed_gate')[1]
    for k in OUTPUTS:
        pipe.out[k].zero()
    pipe.run_fused(block_months=48, mode=1)
    got = pipe.download()
    assert ctx.timing('feed_gate')[1] == n0 + 1, 'the call was not run in the fed order: the paired kernel did not run'
    assert same_bits(got['pet'], ref['pet']), '{} values of PET differ'.format(int((got['pet'] != ref['pet']).sum()))
    for k in ('aet', 'q', 'sav'):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
