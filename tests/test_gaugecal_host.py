"""CPU checks of the gauge form of the streamflow calibration objective (set_calibrate = 1 at stream gauges inside the
network, records with gaps): the numpy restatement against the golden made with the reference's own parts, the gauge
tables (union closures, gauge order, part / join / subset) on hand-built graphs and on the golden world, the two
identities of the contract (a complete record scores as the unmasked formula, one gauge of weight 1 is the basin), the
refusals and the ini keys."""
import logging
from types import SimpleNamespace as NS

import numpy as np
import pytest
import scipy.sparse as sparse

import flowcal_np
import gaugecal_np
from oracle import calib as o_calib, mrtm as o_mrtm
from xanthos_amd.calibrate import gauge_tables as gt
from xanthos_amd.calibrate.calibrate_abcd import Calibrate, calibrate_all
from xanthos_amd.ini_reader import ValidationException


def _um(g):
    return sparse.csr_matrix((g['data'].astype(int), g['indices'], g['indptr']), shape=(g['indptr'].size - 1,) * 2)


def _graph(n, edges):
    """UM = UP - I of a network given as (from, to) edges: row `to` holds +1 at column `from`."""
    r = [t for f, t in edges] + list(range(n))
    c = [f for f, t in edges] + list(range(n))
    v = [1] * len(edges) + [-1] * n
    m = sparse.csr_matrix((v, (r, c)), shape=(n, n))
    m.sort_indices()
    return m


def _world(golden):
    w, g = golden('flowcal'), golden('gaugecal')
    W = {k: w[k] for k in ('basin_ids', 'flow_dist', 'velocity', 'area', 'chs_prev', 'precip', 'tmin', 'pet', 'ndays')}
    W['um'] = _um(w)
    return W, g, int(w['nmonths']), int(w['runoff_spinup']), int(w['routing_spinup'])


def _tables(W, g, tag, nm, rspin, basins=None, **kw):
    gauges = gt.Gauges(g['gauge_id'], g['gauge_cell'], g['gauge_weight'], g[tag + '_obs'])
    return gt.GaugeTables(W['um'], W['basin_ids'], list(g['basins']) if basins is None else basins, gauges,
                          W['flow_dist'], W['velocity'], W['area'], W['chs_prev'], W['ndays'], nm, rspin, **kw)


def _np_args(W, tmin, nm, spin, rspin):
    return (W['um'], W['pet'], W['precip'], tmin, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'], W['ndays'], nm,
            spin, rspin)


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_numpy_restatement_matches_reference_golden(golden, tag):
    W, g, nm, spin, rspin = _world(golden)
    tmin = W['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    for bi, b in enumerate(g['basins']):
        sel = np.nonzero(g['gauge_basin'] == b)[0]
        cells = np.nonzero(W['basin_ids'] == b)[0]
        for j, p in enumerate(g['pars']):
            ed, ed_g, ser = gaugecal_np.objective(p[:npar], g['gauge_cell'][sel], g['gauge_weight'][sel],
                                                  g[tag + '_obs'][sel], cells, *_np_args(W, tmin, nm, spin, rspin))
            ref = g[tag + '_series'][sel, j]
            assert np.all(np.abs(ser - ref) <= 1e-12 * np.abs(ref)), (b, j, np.max(np.abs(ser - ref) / np.abs(ref)))
            ref_e = g[tag + '_ed_gauge'][sel, j]
            assert np.all(np.abs(ed_g - ref_e) <= 1e-12 * np.maximum(1.0, np.abs(ref_e))), (b, j)
            assert abs(ed - g[tag + '_ed'][bi, j]) <= 1e-12 * max(1.0, abs(ed)), (b, j)


def test_golden_gauges_cover_the_corners(golden):
    """Outlet gauges of single-outlet basins, nested gauges with unequal weights, a headwater gauge, foreign closure
    cells, a cell that may fire, multi-outlet basins scored on one gauge, records with the first and last month missing."""
    W, g, nm, spin, rspin = _world(golden)
    w = golden('flowcal')
    t = _tables(W, g, 'snow', nm, rspin)
    ip, ix, sg = gt.um_arrays(W['um'])
    by_id = {int(i): k for k, i in enumerate(t.gauge_id)}
    assert t.gauge_id.tolist() == g['gauge_id'].tolist()                 # the golden is stored in scoring order
    for gid, b in ((101, 2), (102, 6), (103, 9)):
        out, _ = gt.outlets_and_closure(ip, ix, sg, np.nonzero(W['basin_ids'] == b)[0])
        assert out.tolist() == [int(t.gauge_cell[by_id[gid]])] and np.isfinite(t.obs[by_id[gid]]).all()
    lo, up = by_id[104], by_id[105]
    assert t.gauge_basin[lo] == t.gauge_basin[up] and t.gauge_weight[lo] != t.gauge_weight[up]
    clo_of = lambda c: gt.outlets_and_closure(ip, ix, sg, np.array([c]))[1]
    assert t.gauge_cell[up] in clo_of(t.gauge_cell[lo]) and clo_of(t.gauge_cell[up]).size > 1       # nested, interior
    assert clo_of(t.gauge_cell[by_id[108]]).size == 1 and (W['basin_ids'] == 7).sum() > 1           # a headwater gauge
    assert (W['basin_ids'][clo_of(t.gauge_cell[by_id[106]])] == 5).any() and t.gauge_basin[by_id[106]] == 3
    c = t.gauge_cell[by_id[107]]
    assert W['velocity'][c] * float(w['dt']) > W['flow_dist'][c]                                    # may fire
    for b in (1, 5, 7):                                                    # several outlets, scored on a tributary
        out, clo = gt.outlets_and_closure(ip, ix, sg, np.nonzero(W['basin_ids'] == b)[0])
        assert out.size > 1 and t.closures[t.basins.index(b)].size < clo.size
    for k in (104, 105, 106, 107, 108):
        miss = ~np.isfinite(t.obs[by_id[k]])
        assert miss[0] and miss[-1] and 0.15 <= miss.mean() <= 0.25


def test_union_closures_and_gauge_order_on_hand_built_graphs():
    # 0 -> 1 -> 2 -> 6 (ocean);  3 -> 2;  5 -> 3 (a foreign tributary);  4 -> 6;  7 unconnected
    um = _graph(8, [(0, 1), (1, 2), (2, 6), (3, 2), (5, 3), (4, 6)])
    basin_ids = np.array([1, 1, 1, 1, 1, 2, 1, 3])
    nm = 12
    rec = np.arange(1.0, 5 * nm + 1).reshape(5, nm) ** 1.5
    gauges = gt.Gauges([30, 10, 20, 11, 40], [3, 1, 1, 4, 7], [1.0, 2.0, 0.5, 1.0, 1.0], rec)
    L, V, A, S0 = np.arange(1.0, 9.0) * 1000, np.full(8, 0.5), np.arange(8) + 10.0, np.arange(8) * 100.0
    t = gt.GaugeTables(um, basin_ids, [1, 3], gauges, L, V, A, S0, np.full(nm, 30), nm, 3)
    # basin 1: the union of the closures of cells 1, 3 and 4 -- not the outlet closure {0..6}; the foreign cell 5 is in
    assert t.closures[0].tolist() == [0, 1, 3, 4, 5] and t.closures[1].tolist() == [7]
    assert t.closure_ptr.tolist() == [0, 5, 6] and t.gauge_ptr.tolist() == [0, 4, 5]
    # ascending (cell, gauge id): two gauges share cell 1
    assert t.gauge_id.tolist() == [10, 20, 30, 11, 40] and t.gauge_cell.tolist() == [1, 1, 3, 4, 7]
    assert t.gauge_row.tolist() == [1, 1, 2, 3, 0] and t.gauge_weight.tolist() == [2.0, 0.5, 1.0, 1.0, 1.0]
    assert np.array_equal(t.obs, rec[[1, 2, 0, 3, 4]])
    assert t.gauge_basin.tolist() == [1, 1, 1, 1, 3] and t.months_used.tolist() == [nm] * 5
    # forcing columns address ALL of the basin's cells (0, 1, 2, 3, 4, 6): cell 2 and 6 are not in the union
    assert t.basin_col.tolist() == [0, 1, 3, 4, -1, 0]
    c = t.closures[0]
    sub = um[c][:, c].tocsr()
    assert np.array_equal(t.row_ptr[:6], sub.indptr)
    assert np.array_equal(t.cols[:sub.nnz], sub.indices) and np.array_equal(t.sign[:sub.nnz], sub.data)
    assert np.array_equal(t.tauinv, (V / L)[[0, 1, 3, 4, 5, 7]]) and np.array_equal(t.s0, S0[[0, 1, 3, 4, 5, 7]])
    assert t.weights.tolist() == [5 * 15, 1 * 15]                         # union-closure cells x (nmonths + routing_spinup)


def test_part_join_subset_round_trip(golden):
    W, g, nm, spin, rspin = _world(golden)
    t = _tables(W, g, 'snow', nm, rspin)
    names = ('closure_ptr', 'row_ptr', 'cols', 'sign', 'basin_col', 'tauinv', 'area', 's0', 'gauge_ptr', 'gauge_row',
             'gauge_weight', 'gauge_id', 'gauge_cell', 'obs', 'weights', 'ndays')

    def same(a, b):
        assert a.basins == b.basins
        for n in names:
            x, y = getattr(a, n), getattr(b, n)
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), n
        assert all(np.array_equal(p, q) for p, q in zip(a.closures, b.closures))
        assert all(np.array_equal(p, q) for p, q in zip(a.basin_cells, b.basin_cells))
    same(gt.GaugeTables.join([t.part(i) for i in range(len(t.basins))]), t)
    same(t.subset(t.basins), t)
    sub = t.subset([5, 2])
    same(sub, _tables(W, g, 'snow', nm, rspin, basins=[5, 2]))
    assert sub.basins == [5, 2] and sub.gauge_id.tolist() == [105, 104, 101]
    same(sub.part(1), _tables(W, g, 'snow', nm, rspin, basins=[2]))


def test_union_closure_matches_the_world_route(golden):
    """Routing the union closure alone gives the world's Avg_ChFlow at the gauge cells (oracle loops, bit for bit), for
    runoff on all of the basin's cells in the world and on the closure's basin cells only in the closure."""
    W, g, nm, spin, rspin = _world(golden)
    t = _tables(W, g, 'snow', nm, rspin)
    rng = np.random.default_rng(3)
    for i, b in enumerate(t.basins):
        q = np.zeros((W['um'].shape[0], nm))
        q[W['basin_ids'] == b] = rng.uniform(0, 50, ((W['basin_ids'] == b).sum(), nm))
        _, avg, _ = o_mrtm.route_series(W['um'], W['flow_dist'], W['velocity'], W['area'], q, W['ndays'], rspin,
                                        S0=W['chs_prev'])
        p = t.part(i)
        c = p.closures[0]
        sub = sparse.csr_matrix((p.sign.astype(int), p.cols, p.row_ptr), shape=(c.size,) * 2)
        qc = np.where((p.basin_col >= 0)[:, None], q[c], 0.0)
        assert np.array_equal(qc, q[c])                                  # foreign closure cells carry no runoff
        _, avg_c, _ = o_mrtm.route_series(sub, W['flow_dist'][c], W['velocity'][c], p.area, qc, W['ndays'], rspin, S0=p.s0)
        assert np.array_equal(avg_c[p.gauge_row], avg[p.gauge_cell]), b


def test_masked_kge_equals_the_reference_on_compressed_arrays(golden):
    W, g, nm, spin, rspin = _world(golden)
    for tag in ('snow', 'nosnow'):
        for k in range(g['gauge_id'].size):
            for j in range(3):
                got = gaugecal_np.masked_kge_distance(g[tag + '_series'][k, j], g[tag + '_obs'][k])
                assert got == g[tag + '_ed_gauge'][k, j], (tag, k, j)
    # a complete record: the masked score IS the unmasked one
    x, o = g['snow_series'][1, 0], g['snow_obs'][list(g['gauge_id']).index(101)]
    assert gaugecal_np.masked_kge_distance(x, o) == o_calib.kge_distance(x, o)
    # one gauge of weight 1 is the basin
    assert gaugecal_np.combine([0.3721], [1.0]) == 0.3721
    assert gaugecal_np.combine([0.25, 0.5], [2.0, 0.5]) == (2.0 * 0.25 + 0.5 * 0.5) / 2.5


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_complete_outlet_gauge_reproduces_the_outlet_objective(golden, tag):
    """Basins 2, 6 and 9 have one outlet: a complete-record gauge of weight 1 on it gives exactly the series and ED of the
    outlet objective (flowcal_np.objective), and its union closure is the outlet closure."""
    from xanthos_amd.calibrate import flow_tables as ft
    W, g, nm, spin, rspin = _world(golden)
    tmin = W['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    t = _tables(W, g, tag, nm, rspin, basins=[2, 6, 9])
    f = ft.FlowTables(W['um'], W['basin_ids'], [2, 6, 9], W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                      W['ndays'], nm, rspin)
    for name in ('closure_ptr', 'row_ptr', 'cols', 'sign', 'basin_col', 'tauinv', 'area', 's0', 'weights'):
        assert np.array_equal(getattr(t, name), getattr(f, name)), name
    assert np.array_equal(t.gauge_row, np.nonzero(f.outlet_rank == 0)[0] - f.closure_ptr[:-1])
    for i, b in enumerate(t.basins):
        cells = np.nonzero(W['basin_ids'] == b)[0]
        for p in g['pars']:
            args = _np_args(W, tmin, nm, spin, rspin)
            ed, ed_g, ser = gaugecal_np.objective(p[:npar], t.gauge_cell[i:i + 1], [1.0], t.obs[i:i + 1], cells, *args)
            e_out, s_out = flowcal_np.objective(p[:npar], t.obs[i], cells, *args)
            assert np.array_equal(ser[0], s_out) and ed == e_out == ed_g[0]


def test_refusals(golden, caplog):
    W, g, nm, spin, rspin = _world(golden)
    ncell = W['basin_ids'].size
    ids, cells, wts, obs = (g['gauge_id'].copy(), g['gauge_cell'].copy(), g['gauge_weight'].copy(), g['snow_obs'].copy())

    def build(ids=ids, cells=cells, wts=wts, obs=obs, basins=None, **kw):
        return gt.GaugeTables(W['um'], W['basin_ids'], list(g['basins']) if basins is None else basins,
                              gt.Gauges(ids, cells, wts, obs), W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                              W['ndays'], nm, rspin, **kw)
    k = list(ids).index(104)
    c = cells.copy()
    c[k] = ncell
    with pytest.raises(ValidationException, match=r'gauge 104: cell_id {} lies outside the grid of {} cells'.format(
            ncell + 1, ncell)):
        build(cells=c)
    c[k] = -1
    with pytest.raises(ValidationException, match='gauge 104: cell_id 0 lies outside'):
        build(cells=c)
    i2 = ids.copy()
    i2[k] = 101
    with pytest.raises(ValidationException, match='duplicate gauge id 101'):
        build(ids=i2)
    for bad in (0.0, -1.0, np.inf, np.nan):
        w2 = wts.copy()
        w2[k] = bad
        with pytest.raises(ValidationException, match='gauge 104: the weight must be positive and finite'):
            build(wts=w2)
    o2 = obs.copy()
    o2[k] = np.nan
    o2[k, 5] = 3.0
    with pytest.raises(ValidationException, match=r'gauge 104 has 1 finite observation\(s\); the score needs at least 2'):
        build(obs=o2)
    o2[k, 9] = 3.0
    with pytest.raises(ValidationException, match='gauge 104: its finite observations have zero variance'):
        build(obs=o2)
    o2[k, 9] = -3.0
    with pytest.raises(ValidationException, match='gauge 104: its finite observations have zero mean'):
        build(obs=o2)
    # fewer than 12 finite months: a warning, not an error
    o2[k, 9] = 4.0
    o2[k, 11] = 5.0
    with caplog.at_level(logging.WARNING):
        build(obs=o2)
    assert any('gauge 104 has only 3 finite months' in r.getMessage() for r in caplog.records)
    # a calibrated basin without a gauge; gauges of basins that are not calibrated are ignored with one log line
    with pytest.raises(ValidationException, match='basin 8 has no gauge; leave it out of calibration_basins'):
        build(basins=[2, 8])
    caplog.clear()
    with caplog.at_level(logging.INFO):
        t = build(basins=[2, 9])
    assert t.gauge_id.tolist() == [101, 103]
    lines = [r.getMessage() for r in caplog.records if 'not calibrated are ignored' in r.getMessage()]
    assert len(lines) == 1 and '6 gauge(s)' in lines[0] and '104' in lines[0]
    # a union closure larger than the kernel takes; the outlet closure does not matter
    with pytest.raises(ValidationException, match=r'gauges of basin 5 has 89 cells.*at most 64'):
        build(max_closure=64)
    build(basins=[1, 3], max_closure=16)                    # basins 1 and 3 have 178 and 126 cells, their gauges see 9 and 4
    # the existing refusals hold in the gauge form: NaN forcing, a routing spin-up outside the run
    from xanthos_amd.calibrate.calibrate_abcd import flow_tables
    pr = W['precip'].copy()
    pr[np.nonzero(W['basin_ids'] == 2)[0][1], 3] = np.nan
    data = NS(basin_ids=W['basin_ids'], area=W['area'], precip=pr, tmin=None, flow_dist=W['flow_dist'],
              str_velocity=W['velocity'], chs_prev=W['chs_prev'], gauges=gt.Gauges(ids, cells, wts, obs))
    with pytest.raises(ValidationException, match=r'NaN precipitation or PET in basin 2'):
        flow_tables(NS(nmonths=nm, routing_spinup=rspin), data, W['pet'], [2], W['um'], W['ndays'])
    data.precip = W['precip']
    assert flow_tables(NS(nmonths=nm, routing_spinup=rspin), data, W['pet'], [2], W['um'], W['ndays']).gauge_form
    with pytest.raises(ValidationException, match='routing_spinup = 40'):
        flow_tables(NS(nmonths=nm, routing_spinup=40), data, W['pet'], [2], W['um'], W['ndays'])


def test_ini_keys_and_loader(tmp_path):
    from xanthos_amd import synth
    from xanthos_amd.data_load import load_gauges
    from xanthos_amd.ini_reader import ConfigReader
    w = synth.make_world(nrow=12, ncol=24, ncell=120, n_basins=3, seed=2)
    f = synth.make_forcing(w, 36)
    gauges = np.array([[7, 5, 2.0], [3, 60, 1.0]])
    rec = np.arange(1.0, 73.0)
    rec[[0, 40]] = np.nan
    rec[[5, 50]] = -999.0
    gobs = np.stack([np.repeat([7.0, 3.0], 36), np.zeros(72), np.zeros(72), rec], 1)
    ini = synth.write_example(str(tmp_path), w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, gauges=gauges,
                              gauge_obs=gobs, gauge_missing=-999, calibration_basins='1-3')
    c = ConfigReader(ini)
    assert c.calibrate == 1 and c.set_calibrate == 1 and c.obs_unit == 'm3_per_sec' and c.cal_observed is None
    assert c.cal_gauges.endswith('gauges.csv') and c.cal_gauge_observed.endswith('gauge_obs.csv')
    assert c.cal_gauge_missing == -999.0
    g = load_gauges(c.cal_gauges, c.cal_gauge_observed, 36, c.cal_gauge_missing)
    assert g.ids.tolist() == [7, 3] and g.cells.tolist() == [4, 59] and g.weights.tolist() == [2.0, 1.0]
    want = rec.reshape(2, 36).copy()
    want[want == -999.0] = np.nan
    assert np.array_equal(g.obs, want, equal_nan=True) and np.isnan(g.obs).sum() == 4
    # two columns: the default weight is 1
    two = tmp_path / 'two.csv'
    np.savetxt(str(two), gauges[:, :2], delimiter=',', fmt='%.17g')
    assert load_gauges(str(two), c.cal_gauge_observed, 36).weights.tolist() == [1.0, 1.0]
    # misuse: the gauge keys with set_calibrate = 0, and one of the pair without the other
    text = open(ini).read()
    open(ini, 'w').write(text.replace('set_calibrate = 1', 'set_calibrate = 0').replace('m3_per_sec', 'km3_per_mth'))
    with pytest.raises(ValidationException, match=r'gauges, gauge_observed, gauge_missing is valid only with set_calibrate = 1'):
        ConfigReader(ini)
    open(ini, 'w').write('\n'.join(l for l in text.splitlines() if not l.startswith('gauge_observed')))
    with pytest.raises(ValidationException, match='gauges and gauge_observed go together'):
        ConfigReader(ini)
    open(ini, 'w').write('\n'.join(l for l in text.splitlines() if not l.startswith('gauge')))
    with pytest.raises(ValidationException, match='needs observed'):
        ConfigReader(ini)


def test_calibrate_accepts_gauges_until_the_device():
    """The gauge form is accepted and its tables built; without a GPU the search raises HipUnavailable (no fallback)."""
    from xanthos_amd import _hip
    um = _graph(6, [(0, 1), (1, 2), (3, 2), (5, 3)])
    nm = 30
    gauges = gt.Gauges([1], [1], None, (np.arange(nm) + 1.0)[None, :])
    data = NS(basin_ids=np.array([1, 1, 1, 1, 2, 3]), area=np.ones(6), precip=np.ones((6, nm)), tmin=None, cal_obs=None,
              flow_dist=np.full(6, 1e4), str_velocity=np.ones(6), chs_prev=np.zeros(6), gauges=gauges)
    settings = NS(set_calibrate=1, obs_unit='m3_per_sec', cal_basins=['1'], nmonths=nm, runoff_spinup=25,
                  routing_spinup=3, calib_out_dir=None, device=0)
    kw = dict(basin_num=1, basin_ids=data.basin_ids, basin_areas=data.area, precip=data.precip, pet=np.ones((6, nm)),
              obs=None, tmin=None, n_months=nm, runoff_spinup=25, obs_unit='m3_per_sec', out_dir=None, um=um,
              flow_dist=data.flow_dist, velocity=data.str_velocity, ndays=np.full(nm, 30), routing_spinup=3)
    with pytest.raises(ValueError, match='gauges need set_calibrate = 1'):
        Calibrate(set_calibrate=0, gauges=gauges, **kw)
    cal = Calibrate(set_calibrate=1, gauges=gauges, **kw)
    assert cal.flow.gauge_form and cal.flow.closures[0].tolist() == [0, 1] and cal.bsn_Robs is None
    if _hip.device_count() > 0:
        return
    with pytest.raises(_hip.HipUnavailable):
        cal.calibrate_basin()
    with pytest.raises(_hip.HipUnavailable):
        calibrate_all(settings, data, np.ones((6, nm)), um=um, ndays=np.full(nm, 30))
