"""GPU tests (-m gpu) of the one Kling-Gupta distance of csrc/xh_kge.h as its callers expose it: xh_basin_kge (unmasked),
xh_gauge_skill (masked, all eight columns) and xh_calib_objective (the cell-lane calibration's unmasked form).  The same
series against the same record gives the same ED bits from every entry point; the values are numpy's (oracle.calib.kge_distance)
to 1e-9.  Lengths: 2 and 3 (a few lanes busy, the rest idle in the tree), 255 (one lane idle), 256 (exactly full), 257 (one
lane with two terms) and 600 (the model's own)."""
import numpy as np
import pytest

import gaugecal_np
from oracle import calib as o_calib

pytestmark = pytest.mark.gpu

B = 6
LENGTHS = [2, 3, 255, 256, 257, 600]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def case(nmonths):
    """B strictly positive series [B, nmonths] and complete records of their own, neither constant."""
    rng = np.random.default_rng(7100 + nmonths)
    series = rng.gamma(2.0, 150.0, size=(B, nmonths)) + 1.0
    m = np.arange(nmonths)
    obs = np.stack([series[j] * (1.15 + 0.25 * np.sin(2 * np.pi * m / 12.0 + j)) + 5.0 * (m % 2) for j in range(B)])
    assert (series > 0).all() and (obs > 0).all() and (np.ptp(series, axis=1) > 0).all() and (np.ptp(obs, axis=1) > 0).all()
    return series, obs


def basin_kge(ctx, series, obs):
    """ED of xh_basin_kge with one cell per basin and no area: the basin series is 0.0 + x = x."""
    nb, nm = series.shape
    d = [ctx.upload(np.arange(nb + 1), dtype=np.int64), ctx.upload(np.arange(nb), dtype=np.int32), ctx.upload(series),
         ctx.upload(obs), ctx.empty((nb,)), ctx.empty((nb, nm))]
    ctx.basin_kge(nb, nm, nb, d[0], d[1], d[2], None, d[3], d[4], series=d[5])
    ed, ser = d[4].download(), d[5].download()
    for a in d:
        a.free()
    assert np.array_equal(bits(ser), bits(series))                  # what was scored is what was given
    return ed


def gauge_skill(ctx, series, obs):
    """The eight columns of xh_gauge_skill with gauge g on cell g."""
    ng, nm = series.shape
    d = [ctx.upload(np.arange(ng), dtype=np.int32), ctx.upload(series), ctx.upload(obs), ctx.empty((ng, 8))]
    ctx.gauge_skill(ng, nm, ng, d[0], d[1], d[2], d[3])
    got = d[3].download()
    for a in d:
        a.free()
    return got


@pytest.mark.parametrize('nmonths', LENGTHS)
def test_same_series_same_record_same_bits(ctx, nmonths):
    series, obs = case(nmonths)
    ref = np.array([o_calib.kge_distance(s, o) for s, o in zip(series, obs)])
    assert np.all((ref > 1e-3) & (ref < 10.0)), ref                 # a relative bound means something
    ed = basin_kge(ctx, series, obs)
    got = gauge_skill(ctx, series, obs)
    print('nmonths {}: max rel err {:.2e}'.format(nmonths, float(np.max(np.abs(ed - ref) / ref))))
    assert np.array_equal(got[:, 0], np.full(B, float(nmonths)))
    assert np.array_equal(bits(ed), bits(got[:, 1])), (ed, got[:, 1])
    assert np.all(np.abs(ed - ref) <= 1e-9 * ref), (ed, ref)
    assert np.all(np.abs(got[:, 1] - ref) <= 1e-9 * ref), (got[:, 1], ref)


def test_cell_lane_calibration_has_the_bits_of_the_forward_skill(ctx):
    """xh_calib_objective on a 70-cell basin (two chunks) with 3 members -- the cell-lane layout, k_calib_kge -- and
    xh_basin_kge on the series that call returned, one member per basin."""
    ncell, nmem, nm, spin = 70, 3, 36, 25
    rng = np.random.default_rng(7200)
    pet = rng.uniform(20.0, 150.0, (nm, ncell))
    pr = rng.gamma(2.0, 60.0, (nm, ncell)) + 1.0
    pars = np.array([[0.9, 1.6, 0.4, 0.6], [0.7, 3.0, 0.6, 0.3], [0.95, 6.0, 0.2, 0.8]])
    obs = rng.gamma(2.0, 2000.0, nm) + 100.0
    d = [ctx.upload(pet), ctx.upload(pr)]
    ed, series = ctx.calib_objective(ncell, nm, spin, pars, d[0], d[1], None, None, obs, want_series=True)
    for a in d:
        a.free()
    assert series.shape == (nmem, nm) and (series > 0).all() and np.isfinite(ed).all()
    assert len({tuple(bits(s)) for s in series}) == nmem            # three different series
    fwd = basin_kge(ctx, series, np.stack([obs] * nmem))
    assert np.array_equal(bits(ed), bits(fwd)), (ed, fwd)
    ref = np.array([o_calib.kge_distance(s, obs) for s in series])
    assert np.all(np.abs(ed - ref) <= 1e-9 * np.abs(ref)), (ed, ref)


@pytest.mark.parametrize('nmonths', LENGTHS)
def test_masked_equals_unmasked_on_a_complete_record_and_not_on_a_gapped_one(ctx, nmonths):
    series, obs = case(nmonths)
    ed = basin_kge(ctx, series, obs)
    full = gauge_skill(ctx, series, obs)
    assert np.array_equal(bits(full[:, 1]), bits(ed))
    rng = np.random.default_rng(7300 + nmonths)
    gapped = obs.copy()
    ngap = nmonths // 4                                              # 25 % of the months, other months in every record
    for row in gapped:
        row[rng.permutation(nmonths)[:ngap]] = np.nan
    count = np.isfinite(gapped).sum(1)
    assert (count == nmonths - ngap).all() and (count >= 2).all(), count
    got = gauge_skill(ctx, series, gapped)
    ref = np.array([gaugecal_np.masked_kge_distance(s, o) for s, o in zip(series, gapped)])
    assert np.array_equal(got[:, 0], count.astype(float))
    assert np.all(np.abs(got[:, 1] - ref) <= 1e-9 * np.abs(ref)), (got[:, 1], ref)
    if ngap:
        assert (bits(got[:, 1]) != bits(ed)).all(), (got[:, 1], ed)
    else:                                                            # (2 and 3 months: a quarter of them is none)
        assert np.array_equal(bits(got[:, 1]), bits(ed))


def test_degenerate_inputs_give_nan(ctx):
    series, obs = case(36)
    flat = np.full(36, 42.0)
    s = np.stack([flat, series[1]])
    o = np.stack([obs[0], flat])                                     # a constant series; a constant record
    assert np.isnan(basin_kge(ctx, s, o)).all()
    got = gauge_skill(ctx, s, o)
    assert np.array_equal(got[:, 0], [36.0, 36.0]) and np.isnan(got[:, 1]).all()
    one = np.full((1, 36), np.nan)
    one[0, 17] = obs[0, 17]                                          # one finite month: a mean and a bias, no score
    got = gauge_skill(ctx, series[:1], one)
    assert got[0, 0] == 1.0 and np.isnan(got[0, 1:]).all(), got
