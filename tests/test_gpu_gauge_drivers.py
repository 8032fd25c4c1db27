"""GPU tests (-m gpu) of the scoring at stream gauges through the drivers, on a 300-cell, 3-basin, 36-month world: a single
run with [Evaluate] (gauge_flow.csv = the run's own avgchflow rows, gauge_skill.csv = numpy on those rows, every other file
untouched) and an ensemble of parameter tables (every member equal to its single run bit for bit, overlapped = serial, the
hydrographs' statistics equal to numpy, gauges alone with member_outputs = 0, and the basin KGE table unchanged by gauges)."""
import filecmp
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

import ens_np
import gauge_skill_np

pytestmark = pytest.mark.gpu

NM, YEARS = 36, (1971, 1973)
STATS = ('mean', 'std', 'q50')
LB = 1e-4
BOX_LO, BOX_HI = np.full(5, LB), np.array([1 - LB, 8 - LB, 1 - LB, 1 - LB, 1 - LB])
SENTINEL = -999.0
COLUMNS = ('months_used', 'kge', 'r', 'alpha', 'beta', 'nse', 'pbias', 'rmse')


def same_bits(x, ref, tag=''):
    x, ref = np.asarray(x), np.asarray(ref)
    assert x.shape == ref.shape, (tag, x.shape, ref.shape)
    assert np.array_equal(np.isnan(x), np.isnan(ref)), 'NaN masks differ ' + str(tag)
    m = ~np.isnan(ref)
    assert np.array_equal(x[m], ref[m]), '{}: {} of {} values differ'.format(tag, int((x[m] != ref[m]).sum()), int(m.sum()))


def files_of(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            if n != 'logfile.log':
                out[os.path.relpath(os.path.join(base, n), folder)] = os.path.join(base, n)
    return out


def same_files(a, b, tag='', but=()):
    fa, fb = files_of(a), files_of(b)
    for rel in but:
        assert rel in fa, (tag, rel, sorted(fa))
        del fa[rel]
    assert sorted(fa) == sorted(fb) and fa, (tag, sorted(fa), sorted(fb))
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), (tag, rel)


def read_table(path):
    if path.endswith('.npy'):
        return np.load(path)
    rows = open(path).read().splitlines()[1:]
    return np.array([[float(v) if v != '' else np.nan for v in r.split(',')[1:]] for r in rows])


def read_skill(path):
    """gauge_skill.csv -> (header, ids, basins, cell ids, {column: array})."""
    lines = open(path).read().splitlines()
    rows = [r.split(',') for r in lines[1:]]
    cols = {name: np.array([float(r[3 + j]) for r in rows]) for j, name in enumerate(COLUMNS)}
    cols['months_used'] = np.array([int(r[3]) for r in rows])
    return lines[0], [int(r[0]) for r in rows], [int(r[1]) for r in rows], [int(r[2]) for r in rows], cols


def pick_gauges(w, flow):
    """Six gauge cells (0-based) on the world's network, each with a finite hydrograph: the outlet of basin 1 with the most
    cells upstream, a headwater cell, two nested cells on one river (the second upstream of the first), and two more cells
    (the record with gaps, the record with a sentinel)."""
    from xanthos_amd.calibrate.flow_tables import outlets_and_closure, um_arrays
    from xanthos_amd.routing import mrtm
    st = SimpleNamespace(ngridrow=w.nrow, ngridcol=w.ncol)
    um = mrtm.upstream_genmatrix(mrtm.upstream(w.coords, mrtm.downstream(w.coords, w.flow_dir, st), st))
    ip, ix, sg = um_arrays(um)
    closure = [outlets_and_closure(ip, ix, sg, np.array([i]))[1] for i in range(w.ncell)]
    size = np.array([c.size for c in closure])
    ok = np.isfinite(flow).all(1) & (flow.std(1) > 0) & (flow.mean(1) > 1.0)
    basin = np.asarray(w.basin_ids)
    outlets, _ = outlets_and_closure(ip, ix, sg, np.flatnonzero(basin == 1))
    outlets = [int(i) for i in outlets if ok[i]]
    outlet = max(outlets, key=lambda i: size[i])
    heads = [i for i in np.flatnonzero((size == 1) & ok)]
    head = int(max(heads, key=lambda i: flow[i].mean()))
    lower = int(max((i for i in np.flatnonzero(ok & (basin == 2))), key=lambda i: size[i]))
    inner = [int(i) for i in closure[lower] if i != lower and ok[i] and size[i] > 1]
    upper = max(inner, key=lambda i: size[i])
    assert set(closure[upper]) < set(closure[lower])
    rest = [int(i) for i in np.flatnonzero(ok & (basin == 3) & (size > 2)) if i not in (outlet, head, lower, upper)]
    return [outlet, head, lower, upper, rest[0], rest[-1]]


@pytest.fixture(scope='module', params=['pm', 'hargreaves'])
def runs(request, tmp_path_factory):
    """One world per configuration.  The run without [Evaluate]; gauges placed on its network and records made from its own
    avgchflow; the single runs of three parameter tables with [Evaluate]; the resident ensemble overlapped and serial."""
    from xanthos_amd import Xanthos, run_ensemble, synth
    root = str(tmp_path_factory.mktemp('gskill_' + request.param))
    w = synth.make_world(nrow=36, ncol=72, ncell=300, n_basins=3, seed=21)
    f = synth.make_forcing(w, NM, seed=61)
    if request.param == 'pm':
        project, ext = 'pm_abcd_mrtm_synth', 'npy'
        ini = synth.write_example(root, w, f, *YEARS, runoff_spinup=25, routing_spinup=6, output_format=4)
    else:
        project, ext = 'hargreaves_abcd_mrtm_synth', 'csv'
        ini = synth.write_hgm_example(root, w, synth.hgm_forcing(w, f), *YEARS, project=project, runoff='abcd', runoff_spinup=25)
    out = os.path.join(root, 'output', project)
    flow_file = 'avgchflow_m3persec_{}.{}'.format(project, ext)
    plain_ini = shutil.copy(ini, os.path.join(root, 'plain.ini'))
    plain = os.path.join(root, 'single', 'plain')
    c0 = Xanthos(plain_ini).execute({'OutputFolder': plain})
    assert c0.gauge_skill is None and c0.gauge_flow is None
    flow = read_table(os.path.join(plain, flow_file))
    cells = pick_gauges(w, flow)
    ids = [905, 17, 420, 421, 33, 8]                                     # (not sorted: the files keep the order of the gauges file)
    m = np.arange(NM)
    obs = np.stack([flow[c] * (1.15 + 0.25 * np.sin(2 * np.pi * m / 12.0 + j)) for j, c in enumerate(cells)])
    obs[4, [0, 5, 6, 7, 20, 35]] = np.nan                                # gaps
    written = obs.copy()
    written[5, [2, 3, 30]] = SENTINEL                                    # ... and a sentinel
    obs[5, [2, 3, 30]] = np.nan
    synth.enable_evaluate(ini, np.array([[i, c + 1, 1.0 + k] for k, (i, c) in enumerate(zip(ids, cells))]),
                          np.array([[i, 0.0, 0.0, v] for i, row in zip(ids, written) for v in row]), gauge_missing=SENTINEL)
    lo = np.clip(w.abcd_pars * np.array([0.9, 1.1, 0.85, 1.2, 0.95]), BOX_LO, BOX_HI)
    hi = np.clip(w.abcd_pars * np.array([1.05, 0.9, 1.1, 0.8, 1.1]), BOX_LO, BOX_HI)
    lo_file = os.path.join(root, 'pars_lo.npy')
    np.save(lo_file, lo)
    members = [('own', {}), ('lo', {'abcd_pars': lo_file}), ('hi', {'abcd_pars': hi})]
    single, comps = {}, {}
    for name, overrides in members:
        single[name] = os.path.join(root, 'single', name)
        args = {('calib_file' if k == 'abcd_pars' else k): v for k, v in overrides.items()}
        comps[name] = Xanthos(ini).execute(dict(args, OutputFolder=single[name]))
    kw = dict(members=members, statistics=STATS)
    overlapped = run_ensemble(ini, overlap=True, **kw)
    kept = out + '_overlapped'
    os.rename(out, kept)
    serial = run_ensemble(ini, overlap=False, **kw)
    return SimpleNamespace(root=root, world=w, ini=ini, plain_ini=plain_ini, out=out, project=project, ext=ext, members=members,
                           single=single, comps=comps, plain=plain, flow_file=flow_file, cells=cells, ids=ids, obs=obs,
                           overlapped=overlapped, overlapped_out=kept, serial=serial)


# ---- 1. the single run
def test_single_run_writes_the_flow_rows_and_numpy_skill(runs):
    folder, c = runs.single['own'], runs.comps['own']
    flow = read_table(os.path.join(folder, runs.flow_file))
    lines = open(os.path.join(folder, 'gauge_flow.csv')).read().splitlines()
    assert lines[0] == 'gauge_id,' + ','.join('{}{:02}'.format(y, m) for y in range(YEARS[0], YEARS[1] + 1) for m in range(1, 13))
    assert [int(r.split(',')[0]) for r in lines[1:]] == runs.ids
    got_flow = np.array([[float(v) for v in r.split(',')[1:]] for r in lines[1:]])
    same_bits(got_flow, flow[runs.cells], 'gauge_flow.csv')
    same_bits(c.gauge_flow, flow[runs.cells], 'Components.gauge_flow')
    header, ids, basins, cell_ids, cols = read_skill(os.path.join(folder, 'gauge_skill.csv'))
    assert header == 'gauge_id,basin,cell_id,months_used,kge,r,alpha,beta,nse,pbias,rmse'
    assert ids == runs.ids and cell_ids == [i + 1 for i in runs.cells]
    assert basins == [int(runs.world.basin_ids[i]) for i in runs.cells]
    ref = gauge_skill_np.table(gauge_skill_np.skill(flow, runs.cells, runs.obs))
    assert cols['months_used'].tolist() == ref['months_used'].tolist() == [36, 36, 36, 36, 30, 33]
    for name in COLUMNS[1:]:
        assert np.isfinite(ref[name]).all() and np.all((np.abs(ref[name]) >= 0.01) & (np.abs(ref[name]) <= 1000.0)), (name, ref[name])
        err = np.abs(cols[name] - ref[name]) / np.abs(ref[name])
        print('{}: max rel err {:.2e}'.format(name, float(err.max())))
        assert np.all(err <= 1e-9), (name, cols[name], ref[name])
        same_bits(c.gauge_skill[name], cols[name], 'Components.gauge_skill ' + name)
    assert c.gauge_skill['months_used'].tolist() == cols['months_used'].tolist()


def test_evaluate_changes_no_other_file(runs):
    same_files(runs.single['own'], runs.plain, 'with and without [Evaluate]', but=('gauge_skill.csv', 'gauge_flow.csv'))


# ---- 2. the ensemble
def test_members_equal_single_runs(runs):
    res = runs.overlapped
    assert res.names == ['own', 'lo', 'hi'] and res.gauge_ids == runs.ids
    assert res.gauge_kge.shape == (3, 6) and res.gauge_flow.shape == (3, 6, NM)
    assert sorted(res.gauge_skill) == sorted(COLUMNS)
    for k, name in enumerate(res.names):
        c = runs.comps[name]
        same_files(os.path.join(runs.overlapped_out, name), runs.single[name], name)       # the two new files included
        assert 'gauge_skill.csv' in files_of(runs.single[name]) and 'gauge_flow.csv' in files_of(runs.single[name])
        same_bits(res.gauge_kge[k], c.gauge_skill['kge'], name + ' kge')
        for col in COLUMNS:
            same_bits(res.gauge_skill[col][k], c.gauge_skill[col], (name, col))
        same_bits(res.gauge_flow[k], c.gauge_flow, name + ' flow')
    assert not np.array_equal(res.gauge_kge[0], res.gauge_kge[1]) and not np.array_equal(res.gauge_kge[1], res.gauge_kge[2])
    # the two member tables
    folder = os.path.join(runs.overlapped_out, 'ensemble')
    lines = open(os.path.join(folder, 'member_gauge_kge.csv')).read().splitlines()
    assert lines[0] == 'name,' + ','.join(str(i) for i in runs.ids) and [r.split(',')[0] for r in lines[1:]] == res.names
    same_bits(np.array([[float(v) for v in r.split(',')[1:]] for r in lines[1:]]), res.gauge_kge, 'member_gauge_kge.csv')
    lines = open(os.path.join(folder, 'member_gauge_skill.csv')).read().splitlines()
    assert lines[0] == 'name,gauge_id,' + ','.join(COLUMNS) and len(lines) == 1 + 3 * 6
    for k, name in enumerate(res.names):
        single = open(os.path.join(runs.single[name], 'gauge_skill.csv')).read().splitlines()[1:]
        for g, row in enumerate(lines[1 + 6 * k:7 + 6 * k]):
            assert row == ','.join([name, str(runs.ids[g])] + single[g].split(',')[3:]), (name, g)


def test_overlap_changes_no_bit(runs):
    same_files(runs.overlapped_out, runs.out, 'overlap')
    a, b = runs.overlapped, runs.serial
    same_bits(a.gauge_kge, b.gauge_kge, 'kge')
    same_bits(a.gauge_flow, b.gauge_flow, 'flow')
    for col in COLUMNS:
        same_bits(a.gauge_skill[col], b.gauge_skill[col], col)
    for stat in STATS:
        same_bits(a.gauge_flow_statistics[stat], b.gauge_flow_statistics[stat], stat)


def test_hydrograph_statistics_equal_numpy(runs):
    res = runs.overlapped
    stack = np.stack([runs.comps[n].gauge_flow for n in res.names])
    assert sorted(res.gauge_flow_statistics) == sorted(STATS)
    for stat in STATS:
        ref = ens_np.numpy_stat(stack, stat)
        same_bits(res.gauge_flow_statistics[stat], ref, (stat, 'result'))
        same_bits(res.gauge_flow_statistics[stat], ens_np.stat(stack, stat), (stat, 'ens_np'))
        lines = open(os.path.join(runs.overlapped_out, 'ensemble', 'gauge_flow_{}.csv'.format(stat))).read().splitlines()
        assert [int(r.split(',')[0]) for r in lines[1:]] == runs.ids
        same_bits(np.array([[float(v) for v in r.split(',')[1:]] for r in lines[1:]]), ref, (stat, 'file'))
        assert np.isfinite(ref).all()


def test_member_outputs_0_with_gauges_alone_writes_only_the_two_tables(runs):
    from xanthos_amd import run_ensemble
    moved = runs.out + '_serial'
    os.rename(runs.out, moved)
    try:
        res = run_ensemble(runs.ini, members=runs.members, member_outputs=0)
        assert sorted(os.listdir(runs.out)) == ['ensemble', 'logfile.log'] and res.member_dirs == [] and res.statistics == {}
        assert sorted(os.listdir(os.path.join(runs.out, 'ensemble'))) == ['member_gauge_kge.csv', 'member_gauge_skill.csv']
        assert res.gauge_flow_statistics is None and res.kge is None
        same_bits(res.gauge_kge, runs.overlapped.gauge_kge, 'member_outputs = 0')
        same_bits(res.gauge_flow, runs.overlapped.gauge_flow, 'member_outputs = 0, flow')
        for name in ('member_gauge_kge.csv', 'member_gauge_skill.csv'):
            assert filecmp.cmp(os.path.join(runs.out, 'ensemble', name), os.path.join(runs.overlapped_out, 'ensemble', name),
                               shallow=False), name
    finally:
        shutil.rmtree(runs.out, ignore_errors=True)
        os.rename(moved, runs.out)


def test_gauges_leave_the_basin_kge_table_alone(runs):
    from xanthos_amd import ConfigReader, run_ensemble
    basins = sorted(set(int(b) for b in runs.world.basin_ids))
    obs_rows = np.array([[b, 0.0, 0.0, 1.0 + 0.3 * b + 0.5 * np.sin(0.6 * m + b)] for b in basins for m in range(NM)])
    ev = ConfigReader(runs.ini).evaluate
    moved = runs.out + '_serial'
    os.rename(runs.out, moved)
    try:
        kw = dict(members=runs.members, member_outputs=0, observed=obs_rows, obs_unit='km3_per_mth')
        alone = run_ensemble(runs.plain_ini, **kw)
        table = open(os.path.join(runs.out, 'ensemble', 'member_kge.csv')).read()
        assert alone.gauge_kge is None and alone.gauge_ids is None and os.listdir(os.path.join(runs.out, 'ensemble')) == ['member_kge.csv']
        shutil.rmtree(runs.out)
        both = run_ensemble(runs.plain_ini, gauges=ev['gauges'], gauge_observed=ev['gauge_observed'],
                            gauge_missing=ev['gauge_missing'], **kw)                      # (the arguments, not the section)
        same_bits(both.kge, alone.kge, 'kge with and without gauges')
        assert open(os.path.join(runs.out, 'ensemble', 'member_kge.csv')).read() == table
        same_bits(both.gauge_kge, runs.overlapped.gauge_kge, 'gauges by argument')
    finally:
        shutil.rmtree(runs.out, ignore_errors=True)
        os.rename(moved, runs.out)
