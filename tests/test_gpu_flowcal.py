"""GPU tests (-m gpu) of the streamflow calibration objective (set_calibrate = 1; csrc/xh_calib_flow.hip).

The objective is held to the golden made with the reference's own parts (tests/golden/flowcal.npz) and to the numpy
restatement (tests/flowcal_np.py); the device DE on it to oracle/de.py; the search end to end to known parameters.
Small worlds only: every test runs in seconds.
"""
import numpy as np
import pytest
import scipy.sparse as sparse

import flowcal_np

pytestmark = pytest.mark.gpu


def _um(g):
    return sparse.csr_matrix((g['data'].astype(int), g['indices'], g['indptr']), shape=(g['indptr'].size - 1,) * 2)


def _bset(W, basins, tmin, obs, nm, spin, rspin, **kw):
    from xanthos_amd.calibrate.calibrate_abcd import BasinSet, Calibrate
    from xanthos_amd.calibrate.flow_tables import FlowTables
    ft = FlowTables(W['um'], W['basin_ids'], basins, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                    W['ndays'], nm, rspin)
    rows = np.concatenate([np.stack([np.full(nm, b), o[:nm]], 1) for b, o in zip(basins, obs)])
    cals = [Calibrate(basin_num=b, basin_ids=W['basin_ids'], basin_areas=W['area'], precip=W['precip'], pet=W['pet'],
                      obs=rows, tmin=tmin, n_months=nm, runoff_spinup=spin, set_calibrate=1, obs_unit='m3_per_sec',
                      out_dir=kw.get('out_dir'), flow=ft.subset([b]), seed=kw.get('seed')) for b in basins]
    return BasinSet(cals, nm, spin, 'm3_per_sec', flow=ft), ft


@pytest.fixture(scope='module')
def gold(golden):
    g = golden('flowcal')
    W = {k: g[k] for k in ('basin_ids', 'flow_dist', 'velocity', 'area', 'chs_prev', 'precip', 'tmin', 'pet', 'ndays')}
    W['um'] = _um(g)
    return g, W


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_objective_matches_golden_and_numpy(gold, tag):
    """Several basins in one launch (packed-member waves: closures of <= 32 cells, the 1-cell basin, foreign closure
    cells, several outlets, firing cells) against the reference's golden; twice, bit-identical."""
    g, W = gold
    nm, spin, rspin = int(g['nmonths']), int(g['runoff_spinup']), int(g['routing_spinup'])
    tmin = g['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    basins = [int(b) for b in g['basins']]
    bset, ft = _bset(W, basins, tmin, g[tag + '_obs'], nm, spin, rspin)
    assert min(c.size for c in ft.closures) <= 32 < max(c.size for c in ft.closures)
    try:
        nmem = 21                                              # the golden vectors, repeated: several member blocks
        pars = np.stack([g['pars'][np.arange(nmem) % 3, :npar]] * len(basins))
        ed, ser = bset.evaluate(pars, want_series=True)
        ed2, ser2 = bset.evaluate(pars, want_series=True)
    finally:
        bset.close()
    assert np.array_equal(ed, ed2) and np.array_equal(ser, ser2)
    ref_s = g[tag + '_series'][:, np.arange(nmem) % 3]
    ref_e = g[tag + '_ed'][:, np.arange(nmem) % 3]
    assert np.all(np.abs(ser - ref_s) <= 1e-9 * np.abs(ref_s)), np.max(np.abs(ser - ref_s) / np.abs(ref_s))
    assert np.all(np.abs(ed - ref_e) <= 1e-9), np.max(np.abs(ed - ref_e))
    # and the numpy restatement (routes the world) on one basin
    cells = np.nonzero(W['basin_ids'] == 5)[0]
    e_np, s_np = flowcal_np.objective(g['pars'][1, :npar], g[tag + '_obs'][basins.index(5)], cells, W['um'], W['pet'],
                                      W['precip'], tmin, W['flow_dist'], W['velocity'], W['area'], W['chs_prev'],
                                      W['ndays'], nm, spin, rspin)
    assert np.all(np.abs(ser[basins.index(5), 1] - s_np) <= 1e-9 * np.abs(s_np))
    assert abs(ed[basins.index(5), 1] - e_np) <= 1e-9


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


def test_objective_large_closures():
    """Closures of every launch class -- packed waves (<= 32 cells), one wave (33-64), two members per 256-thread
    workgroup (65-128), one (129-256), 2 and 4 cells per lane, 1,024 threads x 3 cells -- with firing cells and closures
    that hold foreign cells, against the numpy restatement."""
    from types import SimpleNamespace
    from oracle import mrtm as o_mrtm, months as o_months
    from xanthos_amd import synth
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
    # tributaries of 65-128, 33-64 and 2-32 cells become basins 5, 6, 7 (their old basins' closures keep them)
    for new, lo, hi in ((5, 65, 128), (6, 33, 64), (7, 2, 32)):
        for i in np.argsort(W['basin_ids'], kind='stable'):
            if W['basin_ids'][i] <= 4:
                t = _subtree(um, int(i))
                if lo <= len(t) <= hi and (W['basin_ids'][t] <= 4).all():
                    W['basin_ids'][t] = new
                    break
    basins = list(range(1, 8))
    pars = np.array([[0.96, 0.8, 0.5, 0.4], [0.7, 2.5, 0.2, 0.8]])
    obs = [np.arange(nm) + 10.0 for _ in basins]
    bset, ft = _bset(W, basins, None, obs, nm, spin, rspin)
    kl = {_klass(c.size) for c in ft.closures}
    assert {(64, 1, 1), (256, 1, 2), (256, 1, 1), (256, 2, 1), (256, 4, 1), (1024, 3, 1)} <= kl, \
        sorted(c.size for c in ft.closures)
    assert any(k[0] == 64 and k[2] >= 2 for k in kl)              # a packed wave of several members
    try:
        ed, ser = bset.evaluate(np.stack([pars] * len(basins)), want_series=True)
    finally:
        bset.close()
    for i, b in enumerate(basins):
        cells = np.nonzero(W['basin_ids'] == b)[0]
        for j in range(2):
            e_np, s_np = flowcal_np.objective(pars[j], obs[i], cells, um, W['pet'], W['precip'], None, fd, W['velocity'],
                                              W['area'], W['chs_prev'], W['ndays'], nm, spin, rspin)
            assert np.all(np.abs(ser[i, j] - s_np) <= 1e-9 * np.abs(s_np)), (b, j)
            assert abs(ed[i, j] - e_np) <= 1e-9, (b, j)


def test_de_generation_on_flow_objective(gold):
    """Trial vectors bit for bit against oracle/de.py, energies equal to a separate evaluation bit for bit."""
    from oracle import de as o_de
    g, W = gold
    nm, spin, rspin = int(g['nmonths']), int(g['runoff_spinup']), int(g['routing_spinup'])
    basins = [1, 3, 9]
    idx = [list(g['basins']).index(b) for b in basins]
    bset, _ = _bset(W, basins, g['tmin'], g['snow_obs'][idx], nm, spin, rspin)
    seed, n, d = 99, 20, 5
    lo, hi = np.array([b[0] for b in bset.bounds]), np.array([b[1] for b in bset.bounds])
    de = bset.solver(n, seed=seed)
    try:
        de.init()
        pop, en = de.state(0)
        for b, key in enumerate(basins):
            assert np.array_equal(pop[b], o_de.init_population(seed, key, n, d))
        assert np.array_equal(en, o_de.clean(bset.evaluate(o_de.scale_parameters(pop, lo, hi))))
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
    """Observations made from known parameters; the device search on the streamflow objective reaches KGE > 0.99."""
    g, W = gold
    nm, spin, rspin = int(g['nmonths']), int(g['runoff_spinup']), int(g['routing_spinup'])
    truth = np.array([0.9, 1.2, 0.4, 0.5])
    cells = np.nonzero(W['basin_ids'] == 1)[0]
    obs = flowcal_np.series(truth, cells, W['um'], W['pet'], W['precip'], None, W['flow_dist'], W['velocity'],
                            W['area'], W['chs_prev'], W['ndays'], nm, spin, rspin)
    bset, _ = _bset(W, [1], None, [obs], nm, spin, rspin, out_dir=str(tmp_path), seed=5)
    cal = bset.cals[0]
    bset.close()
    cal.calibrate_basin()
    assert cal.kge_vals[0] > 0.99, cal.kge_vals
    assert np.load(str(tmp_path / 'kge_result_basin_1.npy'))[0] == cal.kge_vals[0]
    assert np.load(str(tmp_path / 'abcd_parameters_basin_1.npy')).shape == (1, 4)


def test_run_model_streamflow_calibration(tmp_path):
    """run_model() on a synthetic tree with Calibrate = 1, set_calibrate = 1: both files per basin, high KGE."""
    import os
    from types import SimpleNamespace
    from oracle import mrtm as o_mrtm, months as o_months
    from xanthos_amd import Xanthos, synth
    w = synth.make_world(nrow=24, ncol=48, ncell=500, n_basins=6, seed=21)
    nm, spin, rspin = 36, 25, 6
    f = synth.make_forcing(w, nm)
    f['precip'] = np.nan_to_num(f['precip'])
    root = str(tmp_path)
    # observations from known parameters with the PET the run computes
    from xanthos_amd.pet import penman_monteith as pm
    d = synth.data_bag(w, f)
    pet = pm.run_pmpet(d, w.ncell, w.nlcs, 1971, 1973, 0, 6, w.lc_years)
    st = SimpleNamespace(ngridrow=w.nrow, ngridcol=w.ncol)
    um = o_mrtm.upstream_genmatrix(o_mrtm.upstream(w.coords, o_mrtm.downstream(w.coords, w.flow_dir, st), st)).tocsr()
    truth = np.array([0.9, 1.2, 0.4, 0.5, 0.5])
    rows = []
    for b in (1, 2):
        cells = np.nonzero(np.asarray(w.basin_ids) == b)[0]
        s = flowcal_np.series(truth, cells, um, pet, f['precip'], f['abcd_tmin'], w.flow_dist, w.velocity, w.area,
                              np.zeros(w.ncell), o_months.set_month_arrays(nm, 1971, 1973)[:, 2], nm, spin, rspin)
        rows.append(np.stack([np.full(nm, b), np.zeros(nm), np.zeros(nm), s], 1))
    ini = synth.write_example(root, w, f, 1971, 1973, runoff_spinup=spin, routing_spinup=rspin,
                              obs=np.concatenate(rows), set_calibrate=1)
    Xanthos(ini).execute()
    out = os.path.join(root, 'calib_out')
    for b in (1, 2):
        kge = np.load(os.path.join(out, 'kge_result_basin_{}.npy'.format(b)))[0]
        assert kge > 0.99, (b, kge)
        assert np.load(os.path.join(out, 'abcdm_parameters_basin_{}.npy'.format(b))).shape == (1, 5)


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
data = NS(basin_ids=g['basin_ids'], area=g['area'], precip=g['precip'], tmin=g['tmin'], cal_obs=obs,
          flow_dist=g['flow_dist'], str_velocity=g['velocity'], chs_prev=g['chs_prev'])
settings = NS(set_calibrate=1, obs_unit='m3_per_sec', cal_basins=[str(int(b)) for b in g['basins']], nmonths=nm,
              runoff_spinup=int(g['runoff_spinup']), routing_spinup=int(g['routing_spinup']), calib_out_dir=sys.argv[3],
              device=0)
group = launch.current_group()
orig = cal._calibrate_local
def mine(m, *a, **k):
    print('MINE', json.dumps([int(b) for b in m]))
    return orig(m, *a, **k)
cal._calibrate_local = mine
res = cal.calibrate_all(settings, data, g['pet'], seed=11, group=group, um=um, ndays=g['ndays'])
if group is None or group.rank == 0:
    np.save(os.path.join(sys.argv[3], 'res.npy'), np.array([np.append(res[int(b)][0], res[int(b)][1]) for b in g['basins']]))
print('RANK_OK')
"""


def test_two_ranks_equal_one_rank(tmp_path):
    """calibrate_all over 2 ranks on one GPU with a fixed seed: the basins are dealt by closure weight and the parameters
    and KGE are bit-identical to one rank."""
    import os
    import socket
    import subprocess
    import sys
    from xanthos_amd.calibrate.calibrate_abcd import assign_basins
    from xanthos_amd.calibrate.flow_tables import FlowTables
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
        outs[n] = (np.load(str(out / 'res.npy')), texts)
        for b in (1, 2, 3, 5, 9):
            assert (out / 'kge_result_basin_{}.npy'.format(b)).exists()
    assert np.array_equal(outs[1][0], outs[2][0])
    # the dealing follows the closure weights (basin 3's closure holds basin 5's cells)
    import json
    g = np.load(gpath)
    ft = FlowTables(_um(g), g['basin_ids'], list(g['basins']), g['flow_dist'], g['velocity'], g['area'], g['chs_prev'],
                    g['ndays'], int(g['nmonths']), int(g['routing_spinup']))
    owner = assign_basins(ft.weights, 2)
    got = [json.loads(t.split('MINE ')[1].splitlines()[0]) for t in outs[2][1]]
    assert got == [[int(b) for b, r in zip(g['basins'], owner) if r == k] for k in range(2)], got
    assert all(got)
