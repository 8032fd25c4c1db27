"""GPU tests (-m gpu) of the gauge form of the streamflow calibration objective (set_calibrate = 1 at stream gauges;
csrc/xh_calib_flow.hip k_calib_flow<.., GAUGE>, csrc/xh_calib.hip k_calib_kge_masked / k_calib_gauge_combine).

The objective is held to the golden made with the reference's own parts (tests/golden/gaugecal.npz) and to the numpy
restatement (tests/gaugecal_np.py) at the project's tolerances for this objective (series 1e-9 relative, ED 1e-9
absolute), to the outlet form bit for bit where the contract makes them the same, the device DE on it to oracle/de.py,
the search end to end to known parameters.  Small worlds only.
"""
import numpy as np
import pytest
import scipy.sparse as sparse

import gaugecal_np

pytestmark = pytest.mark.gpu


def _um(g):
    return sparse.csr_matrix((g['data'].astype(int), g['indices'], g['indptr']), shape=(g['indptr'].size - 1,) * 2)


def _gset(W, basins, tmin, gauges, nm, spin, rspin, **kw):
    """(BasinSet in gauge form, its GaugeTables) of ``basins`` with the gauges ``gauges`` (gauge_tables.Gauges)."""
    from xanthos_amd.calibrate.calibrate_abcd import BasinSet, Calibrate
    from xanthos_amd.calibrate.gauge_tables import GaugeTables
    t = GaugeTables(W['um'], W['basin_ids'], basins, gauges, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                    W['ndays'], nm, rspin)
    cals = [Calibrate(basin_num=b, basin_ids=W['basin_ids'], basin_areas=W['area'], precip=W['precip'], pet=W['pet'],
                      obs=None, tmin=tmin, n_months=nm, runoff_spinup=spin, set_calibrate=1, obs_unit='m3_per_sec',
                      out_dir=kw.get('out_dir'), flow=t.subset([b]), seed=kw.get('seed')) for b in basins]
    return BasinSet(cals, nm, spin, 'm3_per_sec', flow=t), t


def _np_args(W, tmin, nm, spin, rspin):
    return (W['um'], W['pet'], W['precip'], tmin, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'], W['ndays'], nm,
            spin, rspin)


@pytest.fixture(scope='module')
def gold(golden):
    w, g = golden('flowcal'), golden('gaugecal')
    W = {k: w[k] for k in ('basin_ids', 'flow_dist', 'velocity', 'area', 'chs_prev', 'precip', 'tmin', 'pet', 'ndays')}
    W['um'] = _um(w)
    return g, W, int(w['nmonths']), int(w['runoff_spinup']), int(w['routing_spinup'])


def _golden_gauges(g, tag):
    from xanthos_amd.calibrate.gauge_tables import Gauges
    return Gauges(g['gauge_id'], g['gauge_cell'], g['gauge_weight'], g[tag + '_obs'])


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_objective_matches_golden_and_numpy(gold, tag):
    """Every golden basin in one launch (outlet gauges, nested gauges with unequal weights, a headwater gauge, foreign
    closure cells, a firing cell, records with gaps) against the reference's golden; twice, bit-identical."""
    g, W, nm, spin, rspin = gold
    tmin = W['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    basins = [int(b) for b in g['basins']]
    bset, t = _gset(W, basins, tmin, _golden_gauges(g, tag), nm, spin, rspin)
    assert t.gauge_id.tolist() == g['gauge_id'].tolist()
    try:
        nmem = 21                                              # the golden vectors, repeated: several member blocks
        pars = np.stack([g['pars'][np.arange(nmem) % 3, :npar]] * len(basins))
        ed, ser, edg = bset.evaluate(pars, want_series=True, want_gauges=True)
        ed2, ser2, edg2 = bset.evaluate(pars, want_series=True, want_gauges=True)
        ed3 = bset.evaluate(pars)
    finally:
        bset.close()
    assert np.array_equal(ed, ed2) and np.array_equal(ser, ser2) and np.array_equal(edg, edg2) and np.array_equal(ed, ed3)
    rep = np.arange(nmem) % 3
    ref_s, ref_g, ref_e = g[tag + '_series'][:, rep], g[tag + '_ed_gauge'][:, rep], g[tag + '_ed'][:, rep]
    print('series', np.max(np.abs(ser - ref_s) / np.abs(ref_s)), 'ed_gauge', np.max(np.abs(edg - ref_g)), 'ed',
          np.max(np.abs(ed - ref_e)))
    assert np.all(np.abs(ser - ref_s) <= 1e-9 * np.abs(ref_s)), np.max(np.abs(ser - ref_s) / np.abs(ref_s))
    assert np.all(np.abs(edg - ref_g) <= 1e-9), np.max(np.abs(edg - ref_g))
    assert np.all(np.abs(ed - ref_e) <= 1e-9), np.max(np.abs(ed - ref_e))
    # and the numpy restatement (routes the world) on the basin with the nested gauges
    i = basins.index(5)
    sel = slice(int(t.gauge_ptr[i]), int(t.gauge_ptr[i + 1]))
    e_np, eg_np, s_np = gaugecal_np.objective(g['pars'][1, :npar], t.gauge_cell[sel], t.gauge_weight[sel], t.obs[sel],
                                              np.nonzero(W['basin_ids'] == 5)[0], *_np_args(W, tmin, nm, spin, rspin))
    assert np.all(np.abs(ser[sel, 1] - s_np) <= 1e-9 * np.abs(s_np))
    assert np.all(np.abs(edg[sel, 1] - eg_np) <= 1e-9) and abs(ed[i, 1] - e_np) <= 1e-9


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_complete_outlet_gauge_is_the_outlet_form_bit_for_bit(gold, tag):
    """Basins 2, 6 and 9 have one outlet: a complete-record gauge of weight 1 on it returns exactly the series and ED of
    the outlet form (xh_calib_flow_objective_multi) in the same process."""
    from xanthos_amd.calibrate.calibrate_abcd import BasinSet, Calibrate
    from xanthos_amd.calibrate.flow_tables import FlowTables
    g, W, nm, spin, rspin = gold
    tmin = W['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    basins = [2, 6, 9]
    gset, t = _gset(W, basins, tmin, _golden_gauges(g, tag), nm, spin, rspin)
    ft = FlowTables(W['um'], W['basin_ids'], basins, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                    W['ndays'], nm, rspin)
    rows = np.concatenate([np.stack([np.full(nm, b), o], 1) for b, o in zip(basins, t.obs)])
    cals = [Calibrate(basin_num=b, basin_ids=W['basin_ids'], basin_areas=W['area'], precip=W['precip'], pet=W['pet'],
                      obs=rows, tmin=tmin, n_months=nm, runoff_spinup=spin, set_calibrate=1, obs_unit='m3_per_sec',
                      out_dir=None, flow=ft.subset([b])) for b in basins]
    oset = BasinSet(cals, nm, spin, 'm3_per_sec', flow=ft)
    rng = np.random.default_rng(8)
    lo, hi = np.array([b[0] for b in oset.bounds]), np.array([b[1] for b in oset.bounds])
    try:
        for nmem in (7, 64):                                   # the cell-lane and the member-lane spin-up layouts
            pars = lo + rng.random((len(basins), nmem, npar)) * (hi - lo)
            pars[:, :3] = g['pars'][:, :npar]
            e_g, s_g, eg_g = gset.evaluate(pars, want_series=True, want_gauges=True)
            e_o, s_o = oset.evaluate(pars, want_series=True)
            assert np.array_equal(s_g, s_o), nmem
            assert np.array_equal(e_g, e_o) and np.array_equal(eg_g, e_o), nmem
    finally:
        gset.close()
        oset.close()


def _klass(nc):
    """(threads per workgroup, cells per lane, members per workgroup) of a closure (csrc/xh_calib_flow.hip KLASSES)."""
    for bt, cpl, hi in ((64, 1, 64), (256, 1, 256), (256, 2, 512), (256, 4, 1024), (1024, 3, 3072)):
        if nc <= hi:
            return bt, cpl, (bt // (1 << int(np.ceil(np.log2(nc)))) if cpl == 1 else 1)


def _subtree(um, i):
    up = sparse.csr_matrix(um)
    out, todo = [], [i]
    while todo:
        j = todo.pop()
        out.append(j)
        row = slice(up.indptr[j], up.indptr[j + 1])
        todo.extend(int(c) for c, v in zip(up.indices[row], up.data[row]) if v > 0 and c != j)
    return out


def large_world():
    """The 2,600-cell world of test_gpu_flowcal.test_objective_large_closures (seven basins) with gauges placed so that
    the union closures fall in every launch class: (W, nm, spin, rspin, basins, Gauges).  Basins 1, 4 and 2 get gauges on
    several outlets, whose union closure lies in (1024, 3072], (512, 1024] and (256, 512], basin 3 one interior gauge with
    129-256 cells upstream, basins 5, 6 and 7 (tributaries of 65-128, 33-64 and 2-32 cells) one on their outlet.  The
    weights differ and every record but one has gaps."""
    from types import SimpleNamespace
    from oracle import mrtm as o_mrtm, months as o_months
    from xanthos_amd import synth
    from xanthos_amd.calibrate.gauge_tables import Gauges
    w = synth.make_world(nrow=48, ncol=96, ncell=2600, n_basins=4, seed=17)
    nm, spin, rspin = 26, 25, 2
    f = synth.make_forcing(w, nm)
    st = SimpleNamespace(ngridrow=w.nrow, ngridcol=w.ncol)
    um = o_mrtm.upstream_genmatrix(o_mrtm.upstream(w.coords, o_mrtm.downstream(w.coords, w.flow_dir, st), st)).tocsr()
    rng = np.random.default_rng(5)
    fd = np.asarray(w.flow_dist, dtype=float).copy()
    fire = rng.random(w.ncell) < 0.05
    fd[fire] = w.velocity[fire] * 10800 / rng.uniform(1.5, 4.0, fire.sum())
    W = dict(um=um, basin_ids=np.asarray(w.basin_ids).copy(), flow_dist=fd, velocity=np.asarray(w.velocity, dtype=float),
             area=np.asarray(w.area, dtype=float), chs_prev=rng.uniform(0, 1e6, w.ncell),
             precip=np.nan_to_num(f['precip'][:, :nm]), pet=rng.uniform(20, 150, (w.ncell, nm)),
             ndays=o_months.set_month_arrays(36, 1971, 1973)[:nm, 2])
    roots = {}
    for new, lo, hi in ((5, 65, 128), (6, 33, 64), (7, 2, 32)):
        for i in np.argsort(W['basin_ids'], kind='stable'):
            if W['basin_ids'][i] <= 4:
                t = _subtree(um, int(i))
                if lo <= len(t) <= hi and (W['basin_ids'][t] <= 4).all():
                    W['basin_ids'][t] = new
                    roots[new] = int(i)
                    break
    # basins 1, 4 and 2: gauges on their outlets, the largest subtree first, until the union closure passes 1024, 512
    # and 256 cells (no single cell of this world has more than 482 cells upstream); basin 3: one interior gauge
    from xanthos_amd.calibrate.flow_tables import outlets_and_closure, um_arrays
    ip, ix, sg = um_arrays(um)
    size = np.array([len(_subtree(um, i)) for i in range(w.ncell)])
    cells = []
    for b, lo in ((1, 1024), (4, 512), (2, 256)):
        out, _ = outlets_and_closure(ip, ix, sg, np.nonzero(W['basin_ids'] == b)[0])
        out = [int(i) for i in out[np.argsort(-size[out], kind='stable')] if W['velocity'][i] > 0]
        n = 1
        while outlets_and_closure(ip, ix, sg, np.array(out[:n]))[1].size <= lo:
            n += 1
        cells += out[:n]
    b3 = np.nonzero(W['basin_ids'] == 3)[0]
    cells.append(int(b3[np.argmax(np.where((size[b3] > 128) & (size[b3] <= 256), size[b3], 0))]))
    cells += [roots[b] for b in (5, 6, 7)]
    ids = 200 + np.arange(len(cells))
    weights = 1.0 + (np.arange(len(cells)) % 3)
    obs = 50.0 + 40.0 * np.sin(0.7 * np.arange(nm)[None, :] + ids[:, None]) + np.arange(nm)[None, :]
    miss = np.random.default_rng(23).random(obs.shape) < 0.2
    miss[:, [0, nm - 1]] = True
    miss[1] = False                                            # one complete record
    obs[miss] = np.nan
    return W, nm, spin, rspin, list(range(1, 8)), Gauges(ids, cells, weights, obs)


def test_objective_every_launch_class():
    """Union closures of every launch class -- packed waves (<= 32 cells), one wave (33-64), two members per 256-thread
    workgroup (65-128), one (129-256), 2 and 4 cells per lane, 1,024 threads x 3 cells -- with firing cells, foreign
    closure cells, gaps and basins with several gauges, against the numpy restatement."""
    W, nm, spin, rspin, basins, gauges = large_world()
    pars = np.array([[0.96, 0.8, 0.5, 0.4], [0.7, 2.5, 0.2, 0.8]])
    bset, t = _gset(W, basins, None, gauges, nm, spin, rspin)
    kl = {_klass(c.size) for c in t.closures}
    assert {(64, 1, 1), (256, 1, 2), (256, 1, 1), (256, 2, 1), (256, 4, 1), (1024, 3, 1)} <= kl, \
        sorted(c.size for c in t.closures)
    assert any(k[0] == 64 and k[2] >= 2 for k in kl)              # a packed wave of several members
    assert (np.diff(t.gauge_ptr) > 2).any()
    try:
        ed, ser, edg = bset.evaluate(np.stack([pars] * len(basins)), want_series=True, want_gauges=True)
    finally:
        bset.close()
    worst = [0.0, 0.0, 0.0]
    for i, b in enumerate(basins):
        cells = np.nonzero(W['basin_ids'] == b)[0]
        sel = slice(int(t.gauge_ptr[i]), int(t.gauge_ptr[i + 1]))
        for j in range(2):
            e_np, eg_np, s_np = gaugecal_np.objective(pars[j], t.gauge_cell[sel], t.gauge_weight[sel], t.obs[sel], cells,
                                                      *_np_args(W, None, nm, spin, rspin))
            worst = [max(worst[0], np.max(np.abs(ser[sel, j] - s_np) / np.abs(s_np))),
                     max(worst[1], np.max(np.abs(edg[sel, j] - eg_np))), max(worst[2], abs(ed[i, j] - e_np))]
            assert np.all(np.abs(ser[sel, j] - s_np) <= 1e-9 * np.abs(s_np)), (b, j)
            assert np.all(np.abs(edg[sel, j] - eg_np) <= 1e-9), (b, j)
            assert abs(ed[i, j] - e_np) <= 1e-9, (b, j)
    print('worst series / ed_gauge / ed error', worst)


def test_de_generation_on_gauge_objective(gold):
    """Trial vectors and selection bit for bit against oracle/de.py, energies equal to a separate evaluation bit for bit."""
    from oracle import de as o_de
    g, W, nm, spin, rspin = gold
    basins = [1, 5, 9]
    bset, _ = _gset(W, basins, W['tmin'], _golden_gauges(g, 'snow'), nm, spin, rspin)
    seed, n, d = 99, 20, 5
    lo, hi = np.array([b[0] for b in bset.bounds]), np.array([b[1] for b in bset.bounds])
    de = bset.solver(n, seed=seed)
    try:
        de.init()
        pop, en = de.state(0)
        for b, key in enumerate(basins):
            assert np.array_equal(pop[b], o_de.init_population(seed, key, n, d))
        assert np.array_equal(en, o_de.clean(bset.evaluate(o_de.scale_parameters(pop, lo, hi))))
        assert np.isfinite(en).all()                           # records with gaps no longer poison the energies
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
    finally:
        de.close()
        bset.close()


def test_calibrate_basin_recovers_known_parameters(gold, tmp_path):
    """Observations made from known parameters at two nested gauges with 20 % gaps; the device search on the gauge
    objective reaches KGE > 0.99 at each gauge (the bar the outlet form's recover test sets)."""
    from xanthos_amd.calibrate.gauge_tables import Gauges
    g, W, nm, spin, rspin = gold
    truth = np.array([0.9, 1.2, 0.4, 0.5])
    sel = np.nonzero(g['gauge_basin'] == 5)[0]
    assert sel.size == 2
    avg = gaugecal_np.world_avg(truth, np.nonzero(W['basin_ids'] == 5)[0], *_np_args(W, None, nm, spin, rspin))
    obs = avg[g['gauge_cell'][sel]].copy()
    miss = ~np.isfinite(g['nosnow_obs'][sel])
    assert miss[:, 0].all() and miss[:, -1].all() and 0.15 <= miss.mean() <= 0.25
    obs[miss] = np.nan
    gauges = Gauges(g['gauge_id'][sel], g['gauge_cell'][sel], g['gauge_weight'][sel], obs)
    bset, _ = _gset(W, [5], None, gauges, nm, spin, rspin, out_dir=str(tmp_path), seed=5)
    try:
        cal = bset.cals[0]
        cal.calibrate_basin()
        _, edg = bset.evaluate(cal.all_pars[None, :, :], want_gauges=True)
    finally:
        bset.close()
    kge = 1 - edg[:, 0]
    print('gauge KGE', kge, 'basin KGE', cal.kge_vals)
    assert (kge > 0.99).all(), kge
    assert np.load(str(tmp_path / 'kge_result_basin_5.npy'))[0] == cal.kge_vals[0]
    assert np.load(str(tmp_path / 'abcd_parameters_basin_5.npy')).shape == (1, 4)


def test_run_model_gauge_calibration(tmp_path):
    """run_model() on a synthetic tree with the gauge keys: both files per basin and gauge_kge.csv, high KGE."""
    import os
    from types import SimpleNamespace
    from oracle import mrtm as o_mrtm, months as o_months
    from xanthos_amd import Xanthos, synth
    w = synth.make_world(nrow=24, ncol=48, ncell=500, n_basins=6, seed=21)
    nm, spin, rspin = 36, 25, 6
    f = synth.make_forcing(w, nm)
    f['precip'] = np.nan_to_num(f['precip'])
    root = str(tmp_path)
    from xanthos_amd.pet import penman_monteith as pm
    d = synth.data_bag(w, f)
    pet = pm.run_pmpet(d, w.ncell, w.nlcs, 1971, 1973, 0, 6, w.lc_years)
    st = SimpleNamespace(ngridrow=w.nrow, ngridcol=w.ncol)
    um = o_mrtm.upstream_genmatrix(o_mrtm.upstream(w.coords, o_mrtm.downstream(w.coords, w.flow_dir, st), st)).tocsr()
    bid = np.asarray(w.basin_ids)
    size = np.array([len(_subtree(um, i)) for i in range(w.ncell)])
    truth = np.array([0.9, 1.2, 0.4, 0.5, 0.5])
    ndays = o_months.set_month_arrays(nm, 1971, 1973)[:, 2]
    gauges, rows = [], []
    for b in (1, 2):
        cells = np.nonzero(bid == b)[0]
        avg = gaugecal_np.world_avg(truth, cells, um, pet, f['precip'], f['abcd_tmin'], w.flow_dist, w.velocity, w.area,
                                    np.zeros(w.ncell), ndays, nm, spin, rspin)
        flowing = cells[np.asarray(w.velocity)[cells] > 0]
        main = int(flowing[np.argmax(size[flowing])])
        picks = [(10 * b, main, 2.0)]
        inner = [int(j) for j in _subtree(um, main) if j != main and bid[j] == b and w.velocity[j] > 0 and size[j] >= 3]
        if b == 1 and inner:
            picks.append((10 * b + 1, inner[0], 1.0))           # a nested gauge
        for gid, c, wt in picks:
            s = avg[c].copy()
            s[[0, 7, 19, nm - 1]] = np.nan                      # gaps, half of them written as the sentinel
            rec = np.stack([np.full(nm, gid), np.zeros(nm), np.zeros(nm), s], 1)
            rec[[7, nm - 1], 3] = -9999.0
            rows.append(rec)
            gauges.append((gid, c + 1, wt))
    ini = synth.write_example(root, w, f, 1971, 1973, runoff_spinup=spin, routing_spinup=rspin, gauges=np.array(gauges),
                              gauge_obs=np.concatenate(rows), gauge_missing=-9999.0)
    Xanthos(ini).execute()
    out = os.path.join(root, 'calib_out')
    for b in (1, 2):
        kge = np.load(os.path.join(out, 'kge_result_basin_{}.npy'.format(b)))[0]
        assert kge > 0.99, (b, kge)
        assert np.load(os.path.join(out, 'abcdm_parameters_basin_{}.npy'.format(b))).shape == (1, 5)
    lines = open(os.path.join(out, 'gauge_kge.csv')).read().split()
    assert lines[0] == 'gauge_id,basin,cell_id,months_used,kge' and len(lines) == 1 + len(gauges)
    tab = np.array([[float(x) for x in l.split(',')] for l in lines[1:]])
    want = sorted(gauges, key=lambda r: (bid[r[1] - 1], r[1], r[0]))
    assert tab[:, 0].tolist() == [r[0] for r in want] and tab[:, 2].tolist() == [r[1] for r in want]
    assert tab[:, 1].tolist() == [bid[r[1] - 1] for r in want] and (tab[:, 3] == nm - 4).all()
    assert (tab[:, 4] > 0.99).all(), tab[:, 4]


CALIB_RANK = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, scipy.sparse as sparse
from types import SimpleNamespace as NS
from xanthos_amd import launch
from xanthos_amd.calibrate import calibrate_abcd as cal
from xanthos_amd.calibrate.gauge_tables import Gauges
w, g = np.load(sys.argv[2]), np.load(sys.argv[3])
um = sparse.csr_matrix((w['data'].astype(int), w['indices'], w['indptr']), shape=(w['indptr'].size - 1,) * 2)
nm = int(w['nmonths'])
data = NS(basin_ids=w['basin_ids'], area=w['area'], precip=w['precip'], tmin=w['tmin'], cal_obs=None,
          flow_dist=w['flow_dist'], str_velocity=w['velocity'], chs_prev=w['chs_prev'],
          gauges=Gauges(g['gauge_id'], g['gauge_cell'], g['gauge_weight'], g['snow_obs']))
settings = NS(set_calibrate=1, obs_unit='m3_per_sec', cal_basins=[str(int(b)) for b in g['basins']], nmonths=nm,
              runoff_spinup=int(w['runoff_spinup']), routing_spinup=int(w['routing_spinup']), calib_out_dir=sys.argv[4],
              device=0)
group = launch.current_group()
orig = cal._calibrate_local
def mine(m, *a, **k):
    print('MINE', json.dumps([int(b) for b in m]))
    return orig(m, *a, **k)
cal._calibrate_local = mine
res = cal.calibrate_all(settings, data, w['pet'], seed=11, group=group, um=um, ndays=w['ndays'])
if group is None or group.rank == 0:
    np.save(os.path.join(sys.argv[4], 'res.npy'), np.array([np.append(res[int(b)][0], res[int(b)][1]) for b in g['basins']]))
print('RANK_OK')
"""


def test_two_ranks_equal_one_rank(tmp_path):
    """calibrate_all in gauge form over 2 ranks on one GPU with a fixed seed: the basins are dealt by union-closure weight
    and parameters, KGE and gauge_kge.csv are bit-identical to one rank."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from xanthos_amd.calibrate.calibrate_abcd import assign_basins
    from xanthos_amd.calibrate.gauge_tables import GaugeTables
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
    wpath = os.path.join(root, 'tests', 'golden', 'flowcal.npz')
    gpath = os.path.join(root, 'tests', 'golden', 'gaugecal.npz')
    script = tmp_path / 'rank.py'
    script.write_text(CALIB_RANK)
    g = np.load(gpath)
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
            procs.append(subprocess.Popen([sys.executable, str(script), root, wpath, gpath, str(out)], env=e,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        texts = [p.communicate(timeout=300)[0] for p in procs]
        assert all(p.returncode == 0 and 'RANK_OK' in t for p, t in zip(procs, texts)), [t[-3000:] for t in texts]
        outs[n] = (np.load(str(out / 'res.npy')), texts, (out / 'gauge_kge.csv').read_text())
        for b in g['basins']:
            assert (out / 'kge_result_basin_{}.npy'.format(int(b))).exists()
    assert np.array_equal(outs[1][0], outs[2][0])
    assert outs[1][2] == outs[2][2] and len(outs[1][2].split()) == 1 + g['gauge_id'].size
    # the dealing follows the union-closure weights
    w = np.load(wpath)
    from xanthos_amd.calibrate.gauge_tables import Gauges
    t = GaugeTables(_um(w), w['basin_ids'], list(g['basins']),
                    Gauges(g['gauge_id'], g['gauge_cell'], g['gauge_weight'], g['snow_obs']), w['flow_dist'],
                    w['velocity'], w['area'], w['chs_prev'], w['ndays'], int(w['nmonths']), int(w['routing_spinup']))
    owner = assign_basins(t.weights, 2)
    got = [json.loads(x.split('MINE ')[1].splitlines()[0]) for x in outs[2][1]]
    assert got == [[int(b) for b, r in zip(g['basins'], owner) if r == k] for k in range(2)], got
    assert all(got)
