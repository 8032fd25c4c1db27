"""GPU tests (-m gpu) of xh_gauge_skill through the C-ABI: the eight columns against numpy (gauge_skill_np) on records with
gaps and flow rows with NaNs, the series bit for bit, determinism, the argument errors -- and column 1 (ED) bit for bit
against the per-gauge ED of the calibration's gauge objective (xh_calib_gauge_objective_multi) on the same series and
records."""
from types import SimpleNamespace

import numpy as np
import pytest

import gauge_skill_np

pytestmark = pytest.mark.gpu

NCELL = 500
SHARED, GAPS, ALTERNATE, TWO, NAN_SCORED, NAN_UNSCORED = 137, 250, 251, 300, 400, 401
CELLS = np.array([0, NCELL - 1, SHARED, SHARED, GAPS, ALTERNATE, TWO, NAN_SCORED, NAN_UNSCORED])


def same_bits(x, ref, tag=''):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, tag
    assert np.array_equal(x.view(np.uint64), ref.view(np.uint64)), '{}: {} values differ'.format(
        tag, int((x.view(np.uint64) != ref.view(np.uint64)).sum()))


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def kernel_case(nmonths):
    """(flow [NCELL, nmonths], obs [9, nmonths]): gauges on cell 0 and on the last cell, two on one cell with different
    records, complete records, one with ~30 % scattered gaps, one with every second month missing, one with exactly two
    finite months, one whose flow has a NaN at a scored month and one whose flow has a NaN only where nothing was observed."""
    rng = np.random.default_rng(4000 + nmonths)
    flow = rng.gamma(2.0, 150.0, size=(NCELL, nmonths))
    m = np.arange(nmonths)
    obs = np.stack([flow[c] * (1.15 + 0.25 * np.sin(2 * np.pi * m / 12.0 + j)) for j, c in enumerate(CELLS)])
    obs[4, rng.random(nmonths) < 0.3] = np.nan
    obs[5, 1::2] = np.nan
    keep = np.array([3, nmonths - 2])
    obs[6, np.setdiff1d(m, keep)] = np.nan
    obs[8, rng.random(nmonths) < 0.2] = np.nan
    obs[8, nmonths // 3] = np.nan
    flow[NAN_SCORED, nmonths // 2] = np.nan                          # (observed in that month)
    flow[NAN_UNSCORED, nmonths // 3] = np.nan                        # (not observed in that month)
    assert np.isfinite(obs[7, nmonths // 2]) and np.isfinite(obs[:4]).all() and np.isfinite(obs[6]).sum() == 2
    assert 0 < np.isnan(obs[4]).sum() < nmonths - 2
    return flow, obs


@pytest.mark.parametrize('nmonths', [36, 130, 600])      # below one stride of 256; one stride with a tail; three with a tail
def test_gauge_skill_equals_numpy(ctx, nmonths):
    flow, obs = kernel_case(nmonths)
    ng = len(CELLS)
    ref = gauge_skill_np.skill(flow, CELLS, obs)
    nan_rows = np.isnan(ref[:, 1:]).all(1)
    assert list(np.flatnonzero(nan_rows)) == [7] and not np.isnan(ref[~nan_rows]).any()
    good = ref[~nan_rows, 1:]
    assert np.all((np.abs(good) >= 0.01) & (np.abs(good) <= 1000.0)), ref          # a relative bound means something
    assert np.all(1.0 - ref[~nan_rows, 5] >= 0.04), ref[:, 5]
    d = SimpleNamespace(cells=ctx.upload(CELLS, dtype=np.int32), flow=ctx.upload(flow), obs=ctx.upload(obs),
                        series=ctx.empty((ng, nmonths)), metrics=ctx.empty((ng, 8)))

    def call(series):
        d.metrics.upload(np.full((ng, 8), -1.0))
        ctx.gauge_skill(NCELL, nmonths, ng, d.cells, d.flow, d.obs, d.metrics, series=series)
        return d.metrics.download()
    got = call(d.series)
    series = d.series.download()
    err = np.abs(got[~nan_rows, 1:] - good) / np.abs(good)
    print('nmonths {}: max rel err per column {}'.format(nmonths, ['{:.2e}'.format(e) for e in err.max(0)]))
    assert np.array_equal(got[:, 0], np.isfinite(obs).sum(1)) and np.array_equal(got[:, 0], ref[:, 0])      # months used: exact
    same_bits(series, flow[CELLS], 'series')
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    assert np.all(err <= 1e-9), (got, ref)
    # all-NaN in columns 1..7 exactly where the flow has a NaN at a scored month
    scored_nan = (np.isnan(flow[CELLS]) & np.isfinite(obs)).any(1)
    assert np.array_equal(np.isnan(got[:, 1:]).all(1), scored_nan) and np.array_equal(np.isnan(got[:, 1:]).any(1), scored_nan)
    d.series.upload(np.zeros((ng, nmonths)))
    same_bits(call(d.series), got, 'second call')
    same_bits(d.series.download(), series, 'second call, series')
    same_bits(call(None), got, 'without the series output')
    for a in vars(d).values():
        a.free()


def test_gauge_skill_arguments(ctx):
    from xanthos_amd import _hip
    flow, obs = ctx.upload(np.arange(8.0).reshape(2, 4)), ctx.upload(np.array([[1.0, 3.0, 2.0, 5.0]]))
    cells, metrics = ctx.upload(np.array([1]), dtype=np.int32), ctx.upload(np.zeros((1, 8)))
    good = dict(ncell=2, nmonths=4, ngauge=1, gauge_cell=cells, flow=flow, obs=obs, metrics=metrics)
    for bad in (dict(gauge_cell=None), dict(flow=None), dict(obs=None), dict(metrics=None), dict(ngauge=0), dict(ngauge=-1),
                dict(ngauge=65536), dict(nmonths=1), dict(ncell=0)):
        with pytest.raises(_hip.HipError, match='error {}'.format(_hip.XH_ERR_ARG)):
            ctx.gauge_skill(**dict(good, **bad))
    ctx.gauge_skill(**good)
    row = metrics.download()[0]
    ref = gauge_skill_np.gauge_row(np.arange(4.0, 8.0), np.array([1.0, 3.0, 2.0, 5.0]))
    assert row[0] == 4 and np.all(np.abs(row[1:] - ref[1:]) <= 1e-9 * np.abs(ref[1:])), (row, ref)
    # a cell outside the grid reads nothing and gives NaN (the host refuses it first); one finite month gives NaN
    cells.upload(np.array([2], dtype=np.int32))
    ctx.gauge_skill(**good)
    row = metrics.download()[0]
    assert row[0] == 4 and np.isnan(row[1:]).all()
    cells.upload(np.array([0], dtype=np.int32))
    obs.upload(np.array([[np.nan, 3.0, np.nan, np.nan]]))
    ctx.gauge_skill(**good)
    row = metrics.download()[0]
    assert row[0] == 1 and np.isnan(row[1:]).all()
    for a in (flow, obs, cells, metrics):
        a.free()


# ------------------------------------------------------------------ the same bits as the calibration's gauge objective
def test_ed_has_the_bits_of_the_calibration_gauge_objective(ctx):
    """The per-gauge ED of xh_calib_gauge_objective_multi (k_calib_kge_masked) on a 300-cell world, records with gaps, and
    xh_gauge_skill on the series that call returned, taken as a flow array of ngauge cells: column 1 is the same number."""
    from oracle import months as o_months, mrtm as o_mrtm
    from xanthos_amd import synth
    from xanthos_amd.calibrate.calibrate_abcd import BasinSet, Calibrate
    from xanthos_amd.calibrate.gauge_tables import Gauges, GaugeTables
    import gaugecal_np
    w = synth.make_world(nrow=36, ncol=72, ncell=300, n_basins=3)
    nm, spin, rspin = 36, 25, 6
    f = synth.make_forcing(w, nm)
    st = SimpleNamespace(ngridrow=w.nrow, ngridcol=w.ncol)
    um = o_mrtm.upstream_genmatrix(o_mrtm.upstream(w.coords, o_mrtm.downstream(w.coords, w.flow_dir, st), st)).tocsr()
    rng = np.random.default_rng(31)
    basin_ids = np.asarray(w.basin_ids)
    W = dict(um=um, basin_ids=basin_ids, flow_dist=np.asarray(w.flow_dist, dtype=float), velocity=np.asarray(w.velocity, dtype=float),
             area=np.asarray(w.area, dtype=float), chs_prev=np.zeros(w.ncell), precip=np.nan_to_num(f['precip'][:, :nm]),
             pet=rng.uniform(20, 150, (w.ncell, nm)), ndays=o_months.set_month_arrays(nm, 1971, 1973)[:, 2])
    basins = sorted(set(int(b) for b in basin_ids))
    # three gauges per basin: the cells with the most cells upstream (rows of UM with the most entries)
    upstream = np.diff(um.indptr)
    gcells = np.concatenate([np.flatnonzero(basin_ids == b)[np.argsort(-upstream[basin_ids == b], kind='stable')[:3]]
                             for b in basins])
    ids = 700 + np.arange(gcells.size)
    pars = np.array([0.9, 1.6, 0.4, 0.6])
    obs = np.empty((gcells.size, nm))
    for b in basins:                                               # records: the numpy restatement's series, perturbed
        sel = basin_ids[gcells] == b
        avg = gaugecal_np.world_avg(pars * 0.9, np.flatnonzero(basin_ids == b), um, W['pet'], W['precip'], None, W['flow_dist'],
                                    W['velocity'], W['area'], W['chs_prev'], W['ndays'], nm, spin, rspin)
        obs[sel] = avg[gcells[sel]] * (1.1 + 0.2 * np.sin(0.9 * np.arange(nm)))[None, :] + 1.0
    miss = rng.random(obs.shape) < 0.25
    miss[0] = False                                                # one complete record
    obs[miss] = np.nan
    t = GaugeTables(um, basin_ids, basins, Gauges(ids, gcells, None, obs), W['flow_dist'], W['velocity'], W['area'],
                    W['chs_prev'], W['ndays'], nm, rspin)
    cals = [Calibrate(basin_num=b, basin_ids=basin_ids, basin_areas=W['area'], precip=W['precip'], pet=W['pet'], obs=None,
                      tmin=None, n_months=nm, runoff_spinup=spin, set_calibrate=1, obs_unit='m3_per_sec', out_dir=None,
                      flow=t.subset([b])) for b in basins]
    bset = BasinSet(cals, nm, spin, 'm3_per_sec', flow=t)
    try:
        _, ser, edg = bset.evaluate(np.stack([pars[None, :]] * len(basins)), want_series=True, want_gauges=True)
    finally:
        bset.close()
    ng = int(t.gauge_ptr[-1])
    assert ser.shape == (ng, 1, nm) and edg.shape == (ng, 1) and np.isfinite(edg).all() and np.isnan(t.obs).any()
    assert np.all((edg > 1e-3) & (edg < 10.0)), edg
    d = [ctx.upload(np.arange(ng), dtype=np.int32), ctx.upload(np.ascontiguousarray(ser[:, 0, :])), ctx.upload(t.obs),
         ctx.empty((ng, 8))]
    ctx.gauge_skill(ng, nm, ng, d[0], d[1], d[2], d[3])
    got = d[3].download()
    for a in d:
        a.free()
    assert np.array_equal(got[:, 0], t.months_used)
    same_bits(got[:, 1], edg[:, 0], 'ED against the calibration')
    ref = np.array([gaugecal_np.masked_kge_distance(s, o) for s, o in zip(ser[:, 0], t.obs)])
    assert np.all(np.abs(got[:, 1] - ref) <= 1e-9 * np.abs(ref))
