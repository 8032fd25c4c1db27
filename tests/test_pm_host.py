"""Penman-Monteith on the edge case set, host side (no GPU): the references that tests/test_gpu_pm.py holds the kernel to.

Three statements of the same model are lined up here on tests/pm_cases.py (1,280 one-hot cells x 1994-1996):
  * the real reference's run_pmpet, recorded in tests/golden/pm_edges.npz for five (water_idx, snow_idx) pairs;
  * oracle/pm.py, which must equal it IN BITS (ties of the two indices included: snow is assigned last and reads
    albedo row 6);
  * tests/pm_np.py, the same formulas on np.longdouble, which the device is compared with, and which must agree with the
    other two within the project's Penman-Monteith bar, |x - true| <= 1e-9 |true| + 1e-9 mm.
    Measured: the double reference is at most 1.3e-2 of that bar away from the long-double truth, for every pair (class 5,
    forcing family c: vpd 1e-6 above VPDopen inside a span of 1e-3, 3.6 mm).

The case set is only worth something while it reaches the branches it was built for, so that is asserted, not assumed:
every branch of pm_np.ALL_BRANCHES is taken by at least 8 (cell, month) pairs through the class the cell holds, and at most
0.1 % of the pairs lie within 1e-9 (relative) of one of the two thresholds that are compared with COMPUTED values -- only
those pairs may be left out of the device comparison.
"""
import warnings

import numpy as np
import pytest

import pm_cases
import pm_np
from oracle import pm as o_pm

RTOL, ATOL = 1e-9, 1e-9          # the bar of test_gpu_parity.close and of smoke()


@pytest.fixture(scope='module')
def cs():
    return pm_cases.case_set()


@pytest.fixture(scope='module')
def truth(cs):
    return pm_np.run(cs.data, cs.nlcs, cs.start_year, cs.end_year, cs.lc_years)


def oracle_pet(cs, water_idx, snow_idx):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # 0 / 0 behind np.where, as in the reference
        return o_pm.run_pmpet(cs.data, cs.ncell, cs.nlcs, cs.start_year, cs.end_year, water_idx, snow_idx, cs.lc_years)


def test_case_set_is_the_one_the_reference_ran_on(cs, golden):
    g = golden('pm_edges')
    assert str(g['digest']) == cs.digest, 'tests/pm_cases.py no longer rebuilds the inputs of tests/golden/pm_edges.npz'
    assert (int(g['start_year']), int(g['end_year']), int(g['nlcs'])) == (cs.start_year, cs.end_year, cs.nlcs)
    assert [tuple(p) for p in g['pairs']] == list(pm_cases.INDEX_PAIRS) and list(g['lc_years']) == cs.lc_years
    assert pm_cases.case_set().digest == cs.digest
    # one class per cell and slice, the class moving on with the slice, the fractions cycling
    lct = cs.data.lct_load
    held = (lct > 0).sum(axis=1)
    assert (held[:-pm_cases.ZERO_CELLS] == 1).all() and (held[-pm_cases.ZERO_CELLS:] == 0).all()
    assert set(np.unique(lct[lct > 0])) == set(pm_cases.FRACTIONS)
    assert -400.0 == cs.data.elev.min() and cs.data.elev.max() == 6000.0
    assert np.array_equal(cs.data.tairprev_load[1:], cs.data.tair_load[:-1]) and not cs.data.tairprev_load[0].any()


@pytest.mark.parametrize('pair', pm_cases.INDEX_PAIRS)
def test_oracle_equals_the_reference_in_bits(cs, golden, pair):
    want = pm_cases.golden_pet(golden('pm_edges'), *pair)
    got = oracle_pet(cs, *pair)
    assert got.shape == want.shape and np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        '{} values differ, first at {}'.format(int((got != want).sum()), np.argwhere(got != want)[:1])


@pytest.mark.parametrize('pair', pm_cases.INDEX_PAIRS)
def test_long_double_restatement_agrees_with_the_reference(cs, truth, golden, pair):
    """Worst distance of the double reference from the long-double truth: 1.3e-2 of the bar for each of the five pairs."""
    ref = pm_cases.golden_pet(golden('pm_edges'), *pair)
    true = truth.pet(*pair)
    assert true.dtype == np.longdouble and np.finfo(np.longdouble).eps < 2e-19, 'np.longdouble is not extended precision here'
    assert np.isfinite(true).all()
    ratio = (np.abs(ref - true) / (RTOL * np.abs(true) + ATOL)).astype(np.float64)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print('pair {}: worst {:.3e} of the bar at cell {} month {} (family {}, class {}, PET {:.6g})'.format(
        pair, ratio[at], at[0], at[1], cs.family_names[cs.family[at[0]]], pm_cases.class_by_month(cs)[at], ref[at]))
    assert ratio.max() <= 1.0
    # an exact zero of the truth (the clamps) is an exact zero of the reference
    assert (ref[true == 0] == 0).all()


def test_every_branch_is_reached(cs, truth):
    counts = truth.counts(0, 6)
    print({k: v for k, v in counts.items()})
    assert set(counts) == set(pm_np.ALL_BRANCHES)
    missing = {k: v for k, v in counts.items() if v < 8}
    assert not missing, 'branches the case set no longer reaches (fewer than 8 pairs): {}'.format(missing)
    # every class meets every forcing family in both halves of the year
    klass = pm_cases.class_by_month(cs)
    half = (np.arange(cs.nmonths) % 12 > 5)[None, :]
    for f, name in enumerate(cs.family_names[:-1]):
        rows = cs.family == f
        for l in range(cs.nlcs):
            for h in (False, True):
                assert ((klass[rows] == l) & (half == h)).sum() >= 8, (name, l, h)
    # the edges of the tables are met by the class that carries them
    t = truth.taken
    assert t('gsum_lt_1e-4', 0, 6)[1].sum() >= 8 and (truth.active[1] & ~truth.branches['gsum_lt_1e-4'][1]).sum() >= 8
    assert min(t(n, 0, 6)[2].sum() for n in ('rs_gt_rslimit', 'rhc_gt_rslimit', 'rtot_gt_80', 'ra_gt_rtot', 'rhrc_gt_rtot')) >= 8
    assert min(t(n, 0, 6)[3].sum() for n in ('lai_lt_1e-4', 'lai_le_1e-5', 'lai_fwet_0', 'fc_denom_0', 'fc_0')) >= 8
    assert t('fc_gt_1', 0, 6)[4].sum() >= 8
    assert min(t(n, 0, 6)[5].sum() for n in ('vpd_low', 'vpd_mid', 'vpd_high')) >= 8


@pytest.mark.parametrize('pair', pm_cases.INDEX_PAIRS)
def test_few_cases_sit_on_a_computed_threshold(cs, truth, pair):
    near = truth.near_threshold(*pair)
    print('pair {}: {} of {} (cell, month) pairs within 1e-9 of a computed threshold'.format(pair, int(near.sum()), near.size))
    assert near.sum() <= 1e-3 * near.size
    # family c is a million times further away than the exclusion, and on the side it aims at
    rows = cs.family == cs.family_names.index('c')
    veg = (truth.kinds(*pair) == 'veg')[:, None, None]
    m = truth.margins['vpd'][:, rows][np.broadcast_to(truth.active & veg, truth.active.shape)[:, rows]]
    assert m.size and m.min() > 5e-7 and m.min() < 2e-6
