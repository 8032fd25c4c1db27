"""GPU tests (-m gpu) of the velocity forms of the streamflow calibration objective (calibrate_velocity = 1;
csrc/xh_calib_flow.hip k_calib_flow<.., VEL>), all through the C-ABI's velocity entries.

The objective is held to the golden made with the reference's own parts (tests/golden/velcal.npz) and to the numpy
restatement (tests/velcal_np.py) at the bars of test_gpu_flowcal.py (series 1e-9 relative, ED 1e-9 absolute); to the forms
without the scale bit for bit at v = 1; members to themselves evaluated alone bit for bit in every launch class; the device
DE on it to oracle/de.py; the search to a hidden velocity scale; run_model() end to end, forward with the calibrated scale,
and two ranks to one.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sparse

import flowcal_np
import velcal_np

pytestmark = pytest.mark.gpu

VB = (0.25, 4.0)


def _um(g):
    return sparse.csr_matrix((g['data'].astype(int), g['indices'], g['indptr']), shape=(g['indptr'].size - 1,) * 2)


def _calibrates(W, basins, tmin, rows, nm, spin, tables, vb, **kw):
    from xanthos_amd.calibrate.calibrate_abcd import Calibrate
    return [Calibrate(basin_num=b, basin_ids=W['basin_ids'], basin_areas=W['area'], precip=W['precip'], pet=W['pet'],
                      obs=rows, tmin=tmin, n_months=nm, runoff_spinup=spin, set_calibrate=1, obs_unit='m3_per_sec',
                      out_dir=kw.get('out_dir'), flow=tables.subset([b]), seed=kw.get('seed'), velocity_bounds=vb)
            for b in basins]


def _bset(W, basins, tmin, obs, nm, spin, rspin, vb=VB, **kw):
    """(BasinSet on the outlet form, its FlowTables); vb = None: the form without the scale."""
    from xanthos_amd.calibrate.calibrate_abcd import BasinSet
    from xanthos_amd.calibrate.flow_tables import FlowTables
    ft = FlowTables(W['um'], W['basin_ids'], basins, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                    W['ndays'], nm, rspin)
    rows = np.concatenate([np.stack([np.full(nm, b), o[:nm]], 1) for b, o in zip(basins, obs)])
    return BasinSet(_calibrates(W, basins, tmin, rows, nm, spin, ft, vb, **kw), nm, spin, 'm3_per_sec', flow=ft), ft


def _gset(W, basins, tmin, gauges, nm, spin, rspin, vb=VB, **kw):
    """(BasinSet on the gauge form, its GaugeTables)."""
    from xanthos_amd.calibrate.calibrate_abcd import BasinSet
    from xanthos_amd.calibrate.gauge_tables import GaugeTables
    t = GaugeTables(W['um'], W['basin_ids'], basins, gauges, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                    W['ndays'], nm, rspin)
    return BasinSet(_calibrates(W, basins, tmin, None, nm, spin, t, vb, **kw), nm, spin, 'm3_per_sec', flow=t), t


@pytest.fixture(scope='module')
def gold(golden):
    g, gg, v = golden('flowcal'), golden('gaugecal'), golden('velcal')
    W = {k: g[k] for k in ('basin_ids', 'flow_dist', 'velocity', 'area', 'chs_prev', 'precip', 'tmin', 'pet', 'ndays')}
    W['um'] = _um(g)
    return g, gg, v, W, int(g['nmonths']), int(g['runoff_spinup']), int(g['routing_spinup'])


def _members(v, npar):
    """The golden's (vector, scale) pairs as members [npars * nscales, npar + 1], vector-major."""
    return np.array([np.append(p[:npar], s) for p in v['pars'] for s in v['scales']])


def _close(x, ref, what):
    err = np.max(np.abs(x - ref) / np.abs(ref))
    print(what, 'max relative error', err)
    assert np.all(np.abs(x - ref) <= 1e-9 * np.abs(ref)), (what, err)


def _close_abs(x, ref, what):
    err = np.max(np.abs(x - ref))
    print(what, 'max absolute error', err)
    assert np.all(np.abs(x - ref) <= 1e-9), (what, err)


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_outlet_objective_matches_golden_and_numpy(gold, tag):
    """Every golden basin, vector and scale in one launch against the reference's golden; twice, bit-identical."""
    g, gg, v, W, nm, spin, rspin = gold
    tmin = W['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    basins = [int(b) for b in v['basins']]
    mem = _members(v, npar)
    bset, ft = _bset(W, basins, tmin, v[tag + '_obs'], nm, spin, rspin)
    try:
        pars = np.stack([mem] * len(basins))
        ed, ser = bset.evaluate(pars, want_series=True)
        ed2, ser2 = bset.evaluate(pars, want_series=True)
    finally:
        bset.close()
    assert np.array_equal(ed, ed2) and np.array_equal(ser, ser2)
    _close(ser, v[tag + '_series'].reshape(len(basins), -1, nm), 'outlet series ' + tag)
    _close_abs(ed, v[tag + '_ed'].reshape(len(basins), -1), 'outlet ED ' + tag)
    # the numpy restatement (routes the world) on basin 3, whose closure holds foreign cells, at v = 0.5
    i, j = basins.index(3), 1
    assert mem[j, -1] == 0.5 and ft.part(i).foreign.any()
    e_np, s_np = velcal_np.objective(mem[j], v[tag + '_obs'][i], np.nonzero(W['basin_ids'] == 3)[0], W['um'], W['pet'],
                                     W['precip'], tmin, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                                     W['ndays'], nm, spin, rspin)
    _close(ser[i, j], s_np, 'numpy series')
    assert abs(ed[i, j] - e_np) <= 1e-9


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_gauge_objective_matches_golden_and_numpy(gold, tag):
    from xanthos_amd.calibrate.gauge_tables import Gauges
    g, gg, v, W, nm, spin, rspin = gold
    tmin = W['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    basins = [int(b) for b in v['basins']]
    sel = v['gauge_sel']
    gauges = Gauges(gg['gauge_id'][sel], gg['gauge_cell'][sel], gg['gauge_weight'][sel], v[tag + '_gauge_obs'])
    mem = _members(v, npar)
    bset, t = _gset(W, basins, tmin, gauges, nm, spin, rspin)
    assert t.gauge_id.tolist() == gg['gauge_id'][sel].tolist()
    try:
        pars = np.stack([mem] * len(basins))
        ed, ser, edg = bset.evaluate(pars, want_series=True, want_gauges=True)
        ed2, ser2, edg2 = bset.evaluate(pars, want_series=True, want_gauges=True)
    finally:
        bset.close()
    assert np.array_equal(ed, ed2) and np.array_equal(ser, ser2) and np.array_equal(edg, edg2)
    _close(ser, v[tag + '_gauge_series'].reshape(sel.size, -1, nm), 'gauge series ' + tag)
    _close_abs(edg, v[tag + '_gauge_ed_gauge'].reshape(sel.size, -1), 'ED_g ' + tag)
    _close_abs(ed, v[tag + '_gauge_ed'].reshape(len(basins), -1), 'ED_B ' + tag)
    i, j = basins.index(5), 2
    k = slice(int(t.gauge_ptr[i]), int(t.gauge_ptr[i + 1]))
    e_np, eg_np, s_np = velcal_np.gauge_objective(mem[j], t.gauge_cell[k], t.gauge_weight[k], t.obs[k],
                                                  np.nonzero(W['basin_ids'] == 5)[0], W['um'], W['pet'], W['precip'], tmin,
                                                  W['flow_dist'], W['velocity'], W['area'], W['chs_prev'], W['ndays'], nm,
                                                  spin, rspin)
    _close(ser[k, j], s_np, 'numpy gauge series')
    assert np.all(np.abs(edg[k, j] - eg_np) <= 1e-9) and abs(ed[i, j] - e_np) <= 1e-9


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_foreign_cells_keep_their_velocity(gold, tag):
    """The pin world of the golden: the foreign tributary in basin 3's closure still drains in the scored months, so scaling
    it too would miss the golden by ~9 %; outlet form and the gauge below the tributary."""
    from xanthos_amd.calibrate.gauge_tables import Gauges
    g, gg, v, W, nm, spin, _ = gold
    P = dict(W, flow_dist=v['pin_flow_dist'], velocity=v['pin_velocity'], chs_prev=v['pin_chs_prev'])
    rspin, b = int(v['pin_routing_spinup']), int(v['pin_basin'])
    tmin = W['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    mem = np.array([np.append(p[:npar], s) for p in v['pars'] for s in v['pin_scales']])
    i3 = v['basins'].tolist().index(b)
    bset, ft = _bset(P, [b], tmin, v[tag + '_obs'][i3:i3 + 1], nm, spin, rspin)
    assert ft.foreign.any()
    k = int(v['pin_gauge_index'])
    gauges = Gauges(gg['gauge_id'][k:k + 1], gg['gauge_cell'][k:k + 1], gg['gauge_weight'][k:k + 1], gg[tag + '_obs'][k:k + 1])
    gset, _ = _gset(P, [b], tmin, gauges, nm, spin, rspin)
    try:
        ed, ser = bset.evaluate(mem[None], want_series=True)
        ged, gser = gset.evaluate(mem[None], want_series=True)
    finally:
        bset.close()
        gset.close()
    _close(ser[0], v[tag + '_pin_series'].reshape(-1, nm), 'pin outlet series')
    _close_abs(ed[0], v[tag + '_pin_ed'].reshape(-1), 'pin outlet ED')
    _close(gser[0], v[tag + '_pin_gauge_series'].reshape(-1, nm), 'pin gauge series')
    _close_abs(ged[0], v[tag + '_pin_gauge_ed'].reshape(-1), 'pin gauge ED')


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_unit_scale_is_the_existing_form_bit_for_bit(gold, tag):
    """A v column of exactly 1.0 returns the series and ED of xh_calib_flow_objective_multi and
    xh_calib_gauge_objective_multi; 7 and 64 members: the cell-lane and the member-lane spin-up layouts."""
    from xanthos_amd.calibrate.gauge_tables import Gauges
    g, gg, v, W, nm, spin, rspin = gold
    tmin = W['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    basins = [int(b) for b in v['basins']]
    sel = v['gauge_sel']
    gauges = Gauges(gg['gauge_id'][sel], gg['gauge_cell'][sel], gg['gauge_weight'][sel], v[tag + '_gauge_obs'])
    sets = [_bset(W, basins, tmin, v[tag + '_obs'], nm, spin, rspin, vb=vb)[0] for vb in (VB, None)]
    sets += [_gset(W, basins, tmin, gauges, nm, spin, rspin, vb=vb)[0] for vb in (VB, None)]
    rng = np.random.default_rng(8)
    lo, hi = np.array([b[0] for b in sets[1].bounds]), np.array([b[1] for b in sets[1].bounds])
    try:
        for nmem in (7, 64):
            pars = lo + rng.random((len(basins), nmem, npar)) * (hi - lo)
            pars[:, :2] = v['pars'][:, :npar]
            pv = np.concatenate([pars, np.ones((len(basins), nmem, 1))], axis=2)
            e_v, s_v = sets[0].evaluate(pv, want_series=True)
            e_o, s_o = sets[1].evaluate(pars, want_series=True)
            assert np.array_equal(s_v, s_o) and np.array_equal(e_v, e_o), nmem
            e_v, s_v, g_v = sets[2].evaluate(pv, want_series=True, want_gauges=True)
            e_o, s_o, g_o = sets[3].evaluate(pars, want_series=True, want_gauges=True)
            assert np.array_equal(s_v, s_o) and np.array_equal(e_v, e_o) and np.array_equal(g_v, g_o), nmem
    finally:
        for s in sets:
            s.close()


def test_members_are_independent_in_every_launch_class():
    """A population with mixed v in one launch equals every member evaluated alone, bit for bit: closures of <= 32 cells
    (several members per wave), <= 64, <= 256 (two members per workgroup and one), <= 512, <= 1,024 and > 1,024 cells, the
    outlet form and the gauge form; a sample of members against the numpy restatement."""
    import test_gpu_gaugecal as tg
    W, nm, spin, rspin, basins, gauges = tg.large_world()
    rng = np.random.default_rng(31)
    nmem, npar = 10, 4
    lo, hi = np.array([1e-4, 1e-4, 1e-4, 1e-4, VB[0]]), np.array([1 - 1e-4, 8 - 1e-4, 1 - 1e-4, 1 - 1e-4, VB[1]])
    pars = lo + rng.random((len(basins), nmem, npar + 1)) * (hi - lo)
    pars[:, 0] = [0.96, 0.8, 0.5, 0.4, 0.5]
    pars[:, 1] = [0.7, 2.5, 0.2, 0.8, 2.0]
    pars[:, 2, -1] = 1.0
    obs = [np.arange(nm) + 10.0 for _ in basins]
    bset, ft = _bset(W, basins, None, obs, nm, spin, rspin)
    gset, t = _gset(W, basins, None, gauges, nm, spin, rspin)
    want = {(64, 1, 1), (256, 1, 2), (256, 1, 1), (256, 2, 1), (256, 4, 1), (1024, 3, 1)}
    for tab in (ft, t):
        kl = {tg._klass(c.size) for c in tab.closures}
        assert want <= kl and any(k[0] == 64 and k[2] >= 2 for k in kl), sorted(c.size for c in tab.closures)
    try:
        ed, ser = bset.evaluate(pars, want_series=True)
        ged, gser, gedg = gset.evaluate(pars, want_series=True, want_gauges=True)
        for j in range(nmem):
            e1, s1 = bset.evaluate(pars[:, j:j + 1], want_series=True)
            assert np.array_equal(s1[:, 0], ser[:, j]) and np.array_equal(e1[:, 0], ed[:, j]), j
            e1, s1, g1 = gset.evaluate(pars[:, j:j + 1], want_series=True, want_gauges=True)
            assert np.array_equal(s1[:, 0], gser[:, j]) and np.array_equal(e1[:, 0], ged[:, j]), j
            assert np.array_equal(g1[:, 0], gedg[:, j]), j
    finally:
        bset.close()
        gset.close()
    assert len({tuple(r) for r in ser.reshape(-1, nm)}) == ser.shape[0] * nmem       # the scales do act
    for i, b in enumerate(basins):
        cells = np.nonzero(W['basin_ids'] == b)[0]
        for j in (0, 1):
            e_np, s_np = velcal_np.objective(pars[i, j], obs[i], cells, W['um'], W['pet'], W['precip'], None,
                                             W['flow_dist'], W['velocity'], W['area'], W['chs_prev'], W['ndays'], nm, spin,
                                             rspin)
            assert np.all(np.abs(ser[i, j] - s_np) <= 1e-9 * np.abs(s_np)), (b, j)
            assert abs(ed[i, j] - e_np) <= 1e-9, (b, j)
        k = slice(int(t.gauge_ptr[i]), int(t.gauge_ptr[i + 1]))
        e_np, eg_np, s_np = velcal_np.gauge_objective(pars[i, 1], t.gauge_cell[k], t.gauge_weight[k], t.obs[k], cells,
                                                      W['um'], W['pet'], W['precip'], None, W['flow_dist'], W['velocity'],
                                                      W['area'], W['chs_prev'], W['ndays'], nm, spin, rspin)
        assert np.all(np.abs(gser[k, 1] - s_np) <= 1e-9 * np.abs(s_np)), b
        assert np.all(np.abs(gedg[k, 1] - eg_np) <= 1e-9) and abs(ged[i, 1] - e_np) <= 1e-9, b


@pytest.mark.parametrize('form,tag,d', [('outlet', 'snow', 6), ('gauge', 'nosnow', 5)])
def test_de_generation_on_velocity_objective(gold, form, tag, d):
    """Init, three generations, trial vectors and selection bit for bit against oracle/de.py with d genes; the energies
    equal a separate evaluation bit for bit."""
    from oracle import de as o_de
    from xanthos_amd.calibrate.gauge_tables import Gauges
    g, gg, v, W, nm, spin, rspin = gold
    tmin = W['tmin'] if tag == 'snow' else None
    basins = [1, 3, 9]
    if form == 'outlet':
        idx = [v['basins'].tolist().index(b) for b in basins]
        bset, _ = _bset(W, basins, tmin, v[tag + '_obs'][idx], nm, spin, rspin)
    else:
        sel = v['gauge_sel']
        bset, _ = _gset(W, basins, tmin, Gauges(gg['gauge_id'][sel], gg['gauge_cell'][sel], gg['gauge_weight'][sel],
                                                v[tag + '_gauge_obs']), nm, spin, rspin)
    assert len(bset.bounds) == d and bset.bounds[-1] == VB
    seed, n = 99, 20
    lo, hi = np.array([b[0] for b in bset.bounds]), np.array([b[1] for b in bset.bounds])
    de = bset.solver(n, seed=seed)
    try:
        de.init()
        pop, en = de.state(0)
        assert pop.shape == (3, n, d)
        for b, key in enumerate(basins):
            assert np.array_equal(pop[b], o_de.init_population(seed, key, n, d))
        assert np.array_equal(en, o_de.clean(bset.evaluate(o_de.scale_parameters(pop, lo, hi))))
        assert np.isfinite(en).all()
        for gen in range(3):
            de.step(1, tol=0.01)
            trial, e_trial = de.state(1)
            scaled, _ = de.state(2)
            new_pop, new_en = de.state(0)
            for b, key in enumerate(basins):
                want = o_de.generation_trial(seed, key, gen, pop[b], en[b])
                assert np.array_equal(trial[b], want), (gen, b)
                p2, e2 = o_de.select(pop[b], en[b], want, e_trial[b])
                assert np.array_equal(new_pop[b], p2) and np.array_equal(new_en[b], e2)
            assert np.array_equal(e_trial, bset.evaluate(scaled))
            pop, en = new_pop, new_en
        x, fun, _, _, _ = de.result()
        assert x.shape == (3, d) and np.all((x[:, -1] >= VB[0]) & (x[:, -1] <= VB[1]))
    finally:
        de.close()
        bset.close()


def test_search_recovers_a_hidden_velocity_scale(gold, tmp_path):
    """Observations from the true ABCD parameters with a hidden v = 0.5 on basin 1.  Leaving the velocity alone at the
    true ABCD parameters costs ED >= 0.025 (0.040 measured on the CPU), so KGE > 0.99 needs the scale."""
    g, gg, v, W, nm, spin, rspin = gold
    truth = np.array([0.9, 1.2, 0.4, 0.5, 0.5])
    cells = np.nonzero(W['basin_ids'] == 1)[0]
    args = (cells, W['um'], W['pet'], W['precip'], W['tmin'], W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
            W['ndays'], nm, spin, rspin)
    obs = velcal_np.series(np.append(truth, 0.5), *args)
    ed1, _ = velcal_np.objective(np.append(truth, 1.0), obs, *args)
    print('ED of the true ABCD parameters at v = 1:', ed1)
    assert ed1 >= 0.025, ed1
    out = tmp_path / 'vel'
    bset, _ = _bset(W, [1], W['tmin'], [obs], nm, spin, rspin, out_dir=str(out), seed=5)
    cal = bset.cals[0]
    bset.close()
    cal.calibrate_basin()
    print('with velocity: ED', 1 - cal.kge_vals[0], 'parameters', cal.all_pars[0], 'v', cal.velocity_scale[0], 'nfev', cal.nfev)
    assert cal.kge_vals[0] > 0.99, cal.kge_vals
    assert np.load(str(out / 'kge_result_basin_1.npy'))[0] == cal.kge_vals[0]
    assert np.load(str(out / 'abcdm_parameters_basin_1.npy')).shape == (1, 5)
    assert np.array_equal(np.load(str(out / 'velocity_scale_basin_1.npy')), cal.velocity_scale)
    assert VB[0] <= cal.velocity_scale[0] <= VB[1]
    # the ABCD-only search on the same observations and seed: reported, no order asserted between two stochastic searches
    oset, _ = _bset(W, [1], W['tmin'], [obs], nm, spin, rspin, vb=None, out_dir=str(tmp_path / 'abcd'), seed=5)
    ocal = oset.cals[0]
    oset.close()
    ocal.calibrate_basin()
    print('ABCD only:     ED', 1 - ocal.kge_vals[0], 'parameters', ocal.all_pars[0], 'nfev', ocal.nfev)
    assert not (tmp_path / 'abcd' / 'velocity_scale_basin_1.npy').exists()


def _synthetic_tree():
    from types import SimpleNamespace
    from oracle import mrtm as o_mrtm, months as o_months
    from xanthos_amd import synth
    from xanthos_amd.pet import penman_monteith as pm
    w = synth.make_world(nrow=24, ncol=48, ncell=500, n_basins=6, seed=21)
    nm = 36
    f = synth.make_forcing(w, nm)
    f['precip'] = np.nan_to_num(f['precip'])
    pet = pm.run_pmpet(synth.data_bag(w, f), w.ncell, w.nlcs, 1971, 1973, 0, 6, w.lc_years)
    st = SimpleNamespace(ngridrow=w.nrow, ngridcol=w.ncol)
    um = o_mrtm.upstream_genmatrix(o_mrtm.upstream(w.coords, o_mrtm.downstream(w.coords, w.flow_dir, st), st)).tocsr()
    return w, f, pet, um, o_months.set_month_arrays(nm, 1971, 1973)[:, 2]


def test_run_model_calibrates_velocity_and_runs_forward_with_it(tmp_path):
    """run_model() with calibrate_velocity = 1: every file with its shape, KGE > 0.99; then forward with the calibrated
    calib_file, the written velocity_scale.csv and routing_form = exact: the outlets of a calibrated basin without foreign
    closure cells carry the series of the numpy restatement at the best parameters."""
    from test_gpu_end_to_end import routed_close
    from xanthos_amd import Xanthos, synth
    from xanthos_amd.calibrate.flow_tables import FlowTables
    w, f, pet, um, ndays = _synthetic_tree()
    nm, spin, rspin = 36, 25, 6
    root = str(tmp_path)
    truth, hidden = np.array([0.9, 1.2, 0.4, 0.5, 0.5]), {1: 0.5, 2: 2.0}
    bid = np.asarray(w.basin_ids)
    rows = []
    for b in (1, 2):
        s = velcal_np.series(np.append(truth, hidden[b]), np.nonzero(bid == b)[0], um, pet, f['precip'], f['abcd_tmin'],
                             w.flow_dist, w.velocity, w.area, np.zeros(w.ncell), ndays, nm, spin, rspin)
        rows.append(np.stack([np.full(nm, b), np.zeros(nm), np.zeros(nm), s], 1))
    ini = synth.write_example(root, w, f, 1971, 1973, runoff_spinup=spin, routing_spinup=rspin, obs=np.concatenate(rows),
                              set_calibrate=1, calibrate_velocity=1)
    Xanthos(ini).execute()
    out = os.path.join(root, 'calib_out')
    best = {}
    for b in (1, 2):
        kge = np.load(os.path.join(out, 'kge_result_basin_{}.npy'.format(b)))
        p = np.load(os.path.join(out, 'abcdm_parameters_basin_{}.npy'.format(b)))
        sc = np.load(os.path.join(out, 'velocity_scale_basin_{}.npy'.format(b)))
        assert kge.shape == (1,) and p.shape == (1, 5) and sc.shape == (1,)
        print('basin', b, 'KGE', kge[0], 'parameters', p[0], 'v', sc[0], '(hidden', hidden[b], ')')
        assert kge[0] > 0.99, (b, kge)
        best[b] = np.append(p[0], sc[0])
    lines = open(os.path.join(out, 'velocity_scale.csv')).read().split()
    assert lines[0] == 'basin_id,scale' and len(lines) == 1 + w.n_basins
    tab = [ln.split(',') for ln in lines[1:]]
    assert [int(r[0]) for r in tab] == list(range(1, w.n_basins + 1))
    assert [float(r[1]) for r in tab] == [best[1][-1], best[2][-1]] + [1.0] * (w.n_basins - 2)
    # forward: the calibrated parameters, the written scales, the bit-exact routing form
    rt = os.path.join(root, 'input', 'routing', 'mrtm')
    with open(os.path.join(out, 'velocity_scale.csv')) as src, open(os.path.join(rt, 'velocity_scale.csv'), 'w') as dst:
        dst.write(src.read())
    pars = np.array(w.abcd_pars, dtype=float, copy=True)
    for b in (1, 2):
        pars[b - 1] = best[b][:5]
    np.save(os.path.join(root, 'input', 'runoff', 'abcd', 'pars_calibrated.npy'), pars)
    text = open(ini).read()
    assert 'Calibrate = 1' in text and 'calib_file = pars.npy' in text
    text = text.replace('Calibrate = 1', 'Calibrate = 0').replace('calib_file = pars.npy', 'calib_file = pars_calibrated.npy')
    text = text.replace('flow_direction = flow_dir.npy\n',
                        'flow_direction = flow_dir.npy\nvelocity_scale = velocity_scale.csv\nrouting_form = exact\n')
    fwd = os.path.join(root, 'forward.ini')
    open(fwd, 'w').write(text)
    res = Xanthos(fwd).execute()
    ft = FlowTables(um, bid, [1, 2], w.flow_dist, w.velocity, w.area, None, ndays, nm, rspin)
    clean = [b for i, b in enumerate([1, 2]) if not ft.part(i).foreign.any()]
    assert clean
    raw = np.load(os.path.join(rt, 'velocity.npy'))
    for b in clean:
        cells = np.nonzero(bid == b)[0]
        assert np.array_equal(res.data.str_velocity[cells], raw[cells] * best[b][-1])
        want = velcal_np.series(best[b], cells, um, res.PET, f['precip'], f['abcd_tmin'], res.data.flow_dist, raw,
                                res.data.area, np.zeros(w.ncell), ndays, nm, spin, rspin)
        got = np.zeros(nm)
        for i in flowcal_np.outlets(um, cells):
            got = got + res.Avg_ChFlow[i]
        print('basin', b, 'forward vs numpy', np.max(np.abs(got - want) / np.abs(want)))
        routed_close(got, want, 1e-9, tag='forward outlets of basin {}'.format(b))


def test_forward_run_with_scale_file_equals_prescaled_velocity(tmp_path):
    """run_model() with [[mrtm]] velocity_scale equals run_model() on a tree whose velocity file was multiplied beforehand:
    every array and every output file bit-identical."""
    from xanthos_amd import Xanthos, synth
    from xanthos_amd.calibrate.velocity_scale import cell_scales
    w = synth.make_world(nrow=24, ncol=48, ncell=500, n_basins=6, seed=21)
    f = synth.make_forcing(w, 36)
    scales = {2: 0.37, 5: 2.9}
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    ini_a = synth.write_example(a, w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, velocity_scale=scales)
    full = np.ones(w.n_basins)
    for k, s in scales.items():
        full[k - 1] = s
    from types import SimpleNamespace
    w2 = SimpleNamespace(**vars(w))
    w2.velocity = np.asarray(w.velocity, dtype=float) * cell_scales(w.basin_ids, full)
    assert not np.array_equal(w2.velocity, w.velocity)
    ini_b = synth.write_example(b, w2, f, 1971, 1973, runoff_spinup=25, routing_spinup=6)
    ra, rb = Xanthos(ini_a).execute(), Xanthos(ini_b).execute()
    assert np.array_equal(ra.data.str_velocity, rb.data.str_velocity)
    for name in ('PET', 'AET', 'Q', 'Sav', 'ChStorage', 'Avg_ChFlow'):
        assert np.array_equal(getattr(ra, name), getattr(rb, name), equal_nan=True), name
    oa, ob = (os.path.join(r, 'output', 'pm_abcd_mrtm_synth') for r in (a, b))
    files = sorted(os.listdir(oa))
    assert files and files == sorted(os.listdir(ob))
    outputs = [fn for fn in files if os.path.isfile(os.path.join(oa, fn)) and not fn.endswith('.log')]   # (the log has timings)
    assert len(outputs) >= 2, files
    for fn in outputs:
        assert open(os.path.join(oa, fn), 'rb').read() == open(os.path.join(ob, fn), 'rb').read(), fn
    # and the scale does act: the run without it differs
    r0 = Xanthos(synth.write_example(str(tmp_path / 'c'), w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6)).execute()
    assert not np.array_equal(r0.Avg_ChFlow, ra.Avg_ChFlow, equal_nan=True)


CALIB_RANK = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, scipy.sparse as sparse
from types import SimpleNamespace as NS
from xanthos_amd import launch
from xanthos_amd.calibrate import calibrate_abcd as cal
g = np.load(sys.argv[2])
um = sparse.csr_matrix((g['data'].astype(int), g['indices'], g['indptr']), shape=(g['indptr'].size - 1,) * 2)
nm = int(g['nmonths'])
obs = np.concatenate([np.stack([np.full(nm, b), g['snow_obs'][i]], 1) for i, b in enumerate(g['basins'])])
loaded = np.ones(9)
loaded[[1, 6]] = [1.5, 0.8]
data = NS(basin_ids=g['basin_ids'], area=g['area'], precip=g['precip'], tmin=g['tmin'], cal_obs=obs,
          flow_dist=g['flow_dist'], str_velocity=g['velocity'], chs_prev=g['chs_prev'], velocity_scale=loaded)
settings = NS(set_calibrate=1, obs_unit='m3_per_sec', cal_basins=[str(int(b)) for b in g['basins']], nmonths=nm,
              runoff_spinup=int(g['runoff_spinup']), routing_spinup=int(g['routing_spinup']), calib_out_dir=sys.argv[3],
              device=0, n_basins=9, calibrate_velocity=1, velocity_scale_bounds=(0.25, 4.0))
group = launch.current_group()
res = cal.calibrate_all(settings, data, g['pet'], seed=11, group=group, um=um, ndays=g['ndays'], nmembers=36)
if group is None or group.rank == 0:
    np.save(os.path.join(sys.argv[3], 'res.npy'), np.array([np.append(res[int(b)][0], res[int(b)][1]) for b in g['basins']]))
print('RANK_OK')
"""


def test_two_ranks_equal_one_rank_with_velocity(tmp_path):
    """calibrate_all with the velocity scale over 2 ranks on one GPU with a fixed seed: parameters, scales, KGE and
    velocity_scale.csv are bit-identical to one rank; the csv follows the product rule on the loaded scales."""
    import socket
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
    gpath = os.path.join(root, 'tests', 'golden', 'flowcal.npz')
    script = tmp_path / 'rank.py'
    script.write_text(CALIB_RANK)
    outs = {}
    for n in (1, 2):
        out = tmp_path / str(n)
        out.mkdir()
        env = dict(os.environ)
        for k in ('RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
            env.pop(k, None)
        procs = []
        if n == 2:
            with socket.socket() as sk:
                sk.bind(('127.0.0.1', 0))
                port = sk.getsockname()[1]
        for rank in range(n):
            e = dict(env)
            if n == 2:
                e.update(RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
            procs.append(subprocess.Popen([sys.executable, str(script), root, gpath, str(out)], env=e,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        texts = [p.communicate(timeout=300)[0] for p in procs]
        assert all(p.returncode == 0 and 'RANK_OK' in t for p, t in zip(procs, texts)), [t[-3000:] for t in texts]
        outs[n] = (np.load(str(out / 'res.npy')), (out / 'velocity_scale.csv').read_text(),
                   [np.load(str(out / 'velocity_scale_basin_{}.npy'.format(b))) for b in (1, 2, 3, 5, 9)])
    res = outs[1][0]
    assert res.shape == (5, 7)                                  # a, b, c, d, m, v, KGE
    assert np.array_equal(res, outs[2][0])
    assert outs[1][1] == outs[2][1]
    assert all(np.array_equal(x, y) for x, y in zip(outs[1][2], outs[2][2]))
    from xanthos_amd.calibrate.velocity_scale import read_velocity_scale
    got = read_velocity_scale(str(tmp_path / '1' / 'velocity_scale.csv'), 9)
    want = np.ones(9)
    want[[1, 6]] = [1.5, 0.8]
    for b, v in zip((1, 2, 3, 5, 9), res[:, 5]):
        want[b - 1] = want[b - 1] * v
        assert 0.25 <= v <= 4.0
    assert np.array_equal(got, want)
