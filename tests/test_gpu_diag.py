"""GPU tests of the diagnostics and time-series post-processors (csrc/xh_diag.hip, xh_agg_spatial) against the reference's
golden vectors, the restatements of tests/diag_np.py, whole model runs (one rank and two) and a full-size run."""
import io
import os
import subprocess
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_np as D  # noqa: E402

from xanthos_amd import _hip, synth  # noqa: E402
from xanthos_amd.diagnostics import diagnostics, time_series  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
FAKE = os.path.join(ROOT, 'tests', 'fake_rccl')
LENGTHS = (1, 7, 8, 9, 127, 128, 129, 136, 300)
SCALES = ('Basin', 'Country', 'Region')


def _csv_text(df):
    buf = io.StringIO()
    df.to_csv(buf, na_rep=0, index=False)
    return buf.getvalue()


def _recorder(monkeypatch, root):
    calls = []

    def rec(data, outputname, qstr, TimeUnit, LengthUnit, X):
        assert len(X['data']) == len(data)
        calls.append((os.path.relpath('{0}_{1}.png'.format(outputname, qstr), root), np.array(data)))
    monkeypatch.setattr(time_series, 'Plot_TS', rec)
    return calls


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('ncols', [1, 7, 8, 127, 128, 129, 136, 600, 720, 1201, 9000])
def test_cell_totals_are_numpy_sum(ncols):
    rng = np.random.default_rng(ncols)
    ncell = 700
    a = rng.standard_normal((ncell, ncols)) * 10.0 ** rng.integers(-6, 9, (ncell, ncols))
    a[3, ncols // 2] = np.nan
    a[4, 0] = np.inf
    a[5] = -0.0
    area = rng.uniform(100.0, 3000.0, ncell)
    ctx = _hip.get_context(0)
    d_a, d_area, d_out = ctx.upload(a), ctx.upload(area), ctx.empty((ncell, 2))
    ctx.diag_cell_total(ncell, ncols, d_a, 1.0, None, 1.0, d_out, 2)
    ctx.diag_cell_total(ncell, ncols, d_a, 3.0, d_area, 1e6, d_out.ptr + 8, 2)
    out = d_out.download()
    for b in (d_a, d_area, d_out):
        b.free()
    want = np.sum(a, axis=1)
    assert np.array_equal(out[:, 0], want, equal_nan=True) and not np.signbit(out[5, 0])
    assert np.array_equal(out[:, 1], want / 3 * area / 1e6, equal_nan=True)


def test_group_sums_are_pandas_on_a_cancellation():
    rng = np.random.default_rng(9)
    n, k = 5000, 3
    v = rng.standard_normal((n, k))
    ids = rng.integers(0, 6, n)
    g2 = np.flatnonzero(ids == 2)
    v[g2[:4], 0] = [1e16, 1.0, 1.0, -1e16]              # compensated: 2 survives; a plain sum loses it
    v[g2[5], 1], v[g2[6], 2], v[g2[7], 2] = np.nan, np.inf, 1.0
    ids[ids == 4] = 3                                     # an id without cells inside the dense range
    ctx = _hip.get_context(0)
    d_v, d_s, d_c = ctx.upload(v), ctx.empty((6, k)), ctx.empty((6,), dtype=np.int64)
    ctx.diag_group_sum(n, k, 6, ids.astype(np.int32), d_v, d_s, d_c)
    s, c = d_s.download(), d_c.download()
    for b in (d_v, d_s, d_c):
        b.free()
    df = pd.DataFrame(v)
    df['id'] = ids
    want = df.groupby('id').sum()
    assert np.array_equal(c, np.bincount(ids, minlength=6)) and c[4] == 0 and (s[4] == 0).all()
    assert np.array_equal(s[want.index.values], want.values, equal_nan=True)
    plain = np.zeros(k)
    for x in v[g2, 0]:
        plain[0] += x
    assert s[2, 0] != plain[0]


@pytest.mark.parametrize('n', LENGTHS)
def test_diagnostics_write_the_reference_csvs(golden, tmp_path, n):
    g = golden('diag')
    ref = SimpleNamespace(**{k: g['k_' + k] for k in ('area', 'basin_ids', 'country_ids', 'region_ids', 'vic', 'unh',
                                                     'wbmd', 'wbmc', 'basin_names', 'country_names', 'region_names')})
    y0, y1 = g['k{}_years'.format(n)]
    s = SimpleNamespace(PerformDiagnostics=1, OutputFolder=str(tmp_path), StartYear=int(y0), EndYear=int(y1),
                        DiagnosticScale=0, device=0)
    ctx = _hip.get_context(0)
    d_q = ctx.upload(np.ascontiguousarray(g['k_q'][:, :n]))
    diagnostics.Diagnostics(s, d_q, ref)
    d_q.free()
    for sc in SCALES:
        text = open(os.path.join(str(tmp_path), diagnostics.FILE.format(sc))).read()
        assert text == str(g['k{}_{}_csv'.format(n, sc)]), sc


def test_time_series_tables_and_plots_equal_the_reference(golden, tmp_path, monkeypatch):
    g = golden('diag')
    ref = SimpleNamespace(**{k: g['ts_' + k] for k in ('basin_ids', 'country_ids', 'region_ids', 'basin_names',
                                                       'country_names', 'region_names')})
    assert np.array_equal(time_series.Aggregation_Map(ref.basin_ids, g['ts_q']), g['ts_basin_table'])
    assert np.array_equal(time_series.Aggregation_Map(ref.country_ids, g['ts_q']), g['ts_country_table'])
    calls = _recorder(monkeypatch, str(tmp_path))
    s = SimpleNamespace(CreateTimeSeriesPlot=1, OutputFolder=str(tmp_path), TimeSeriesMapID=999, TimeSeriesScale=0,
                        OutputInYear=1, OutputUnit=0, StartYear=1971, EndYear=1994, device=0)
    time_series.TimeSeriesPlot(s, g['ts_q'], g['ts_ac'], ref)
    names = [str(p) for p in g['ts_plot_names']]
    assert [c[0] for c in calls] == names
    assert np.array_equal(np.stack([c[1] for c in calls]), g['ts_plot_data'])


# ---------------------------------------------------------------------------------------------- whole model runs
def _tree(golden, tmp_path):
    g = golden('diag')
    root = str(tmp_path)
    with zipfile.ZipFile(io.BytesIO(g['model_tree_zip'].tobytes())) as z:
        z.extractall(root)
    ini = os.path.join(root, str(g['model_ini_name']))
    text = open(ini).read().replace(str(g['model_old_root']), root)
    open(ini, 'w').write(text)
    return g, ini


def _csv_close(a_path, b_text, rtol):
    a = pd.read_csv(a_path)
    b = pd.read_csv(io.StringIO(b_text))
    assert list(a.columns) == list(b.columns) and a.shape == b.shape and (a['name'] == b['name']).all()
    x, y = a.iloc[:, 1:].values, b.iloc[:, 1:].values
    assert (np.abs(x - y) <= rtol * np.abs(y) + 1e-300).all(), float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))


def test_model_run_hargreaves_gwam_matches_the_reference(golden, tmp_path, monkeypatch):
    from xanthos_amd.model import Xanthos
    g, ini = _tree(golden, tmp_path)
    od = os.path.join(str(tmp_path), 'output', 'hargreaves_gwam_mrtm_synth')
    calls = _recorder(monkeypatch, od)
    c = Xanthos(ini).execute()
    assert c.pipe is not None and 'Q' not in c._host and 'Avg_ChFlow' not in c._host      # read in HBM
    # the run's runoff agrees with the reference's to rounding: the csvs are compared as numbers, and the
    # reference's own Q through this package gives its csv texts exactly
    for sc in SCALES:
        _csv_close(os.path.join(od, diagnostics.FILE.format(sc)), str(g['model_{}_csv'.format(sc)]), 1e-9)
    diagnostics.Diagnostics(SimpleNamespace(PerformDiagnostics=1, OutputFolder=str(tmp_path / 'refq'), StartYear=1971,
                                            EndYear=1972, DiagnosticScale=0, device=0), g['model_Q'], c._diag_maps())
    for sc in SCALES:
        assert open(os.path.join(str(tmp_path / 'refq'), diagnostics.FILE.format(sc))).read() == \
            str(g['model_{}_csv'.format(sc)]), sc
    assert sorted(c[0] for c in calls) == sorted(str(p) for p in g['model_plot_names'])
    want = dict(zip((str(p) for p in g['model_plot_names']), g['model_plot_data']))
    for name, data in calls:
        np.testing.assert_allclose(data, want[name], rtol=1e-9, atol=1e-300, err_msg=name)


def test_model_run_pm_abcd_writes_the_numpy_tables_and_plots(tmp_path, monkeypatch):
    from xanthos_amd.model import Xanthos
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=31)
    f = synth.make_forcing(w, 36)
    root = str(tmp_path)
    ini = synth.write_example(root, w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, aggregates=True,
                              output_in_year=1)
    synth.write_diag_inputs(root, w)
    synth.enable_diagnostics(ini, diag_scale=0, plot_scale=0, map_id=[0, 2, 3])
    od = os.path.join(root, 'output', 'pm_abcd_mrtm_synth')
    calls = _recorder(monkeypatch, od)
    c = Xanthos(ini).execute()
    tables = D.diag_tables(c.Q, 3, c.data)
    for sc in SCALES:
        assert open(os.path.join(od, diagnostics.FILE.format(sc))).read() == _csv_text(tables[sc]), sc
    q, ac = c.q, c.ac
    assert q.shape == (900, 3)
    want = []
    for sc, attr in (('Basin', 'basin'), ('Country', 'country'), ('GCAMRegion', 'region')):
        ids, names = getattr(c.data, attr + '_ids'), np.insert(getattr(c.data, attr + '_names'), 0, 'Global')
        tq, ta = (time_series.with_global(D.aggregation(ids, x)) for x in (q, ac))
        for i in (0, 2, 3):
            stem = os.path.join('TimeSeriesPlot', sc, '{}{}_{}'.format(sc, i, names[i]))
            want += [(stem + '_runoff.png', tq[i]), (stem + '_streamflow.png', ta[i])]
    assert [x[0] for x in calls] == [x[0] for x in want]
    for (_, a), (_, b) in zip(calls, want):
        assert np.array_equal(a, b)


RUN_MODEL_PARENT = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
from xanthos_amd import run_model
res = run_model(sys.argv[2], gpus=int(sys.argv[3]))
print('PARENT_OK')
'''


def test_two_ranks_write_the_same_diagnostics_csvs(tmp_path):
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=33)
    f = synth.make_forcing(w, 36, nan_precip=False)
    fake = os.path.join(FAKE, 'librccl.so.1')
    if not os.path.isfile(fake):
        subprocess.run(['make', '-C', FAKE], check=True, capture_output=True)
    outs = {}
    for tag, n in (('one', 1), ('two', 2)):
        root = str(tmp_path / tag)
        os.makedirs(root)
        ini = synth.write_example(root, w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, output_vars=('q',),
                                  aggregates=True)
        text = open(ini).read().replace('routing_spinup', 'routing_form = exact\n    routing_spinup', 1)
        open(ini, 'w').write(text)
        synth.write_diag_inputs(root, w, seed=23)
        synth.enable_diagnostics(ini, diag_scale=0, plots=False)
        script = tmp_path / (tag + '.py')
        script.write_text(RUN_MODEL_PARENT)
        env = dict(os.environ)
        env.update({'XH_ONE_DEVICE': '1', 'XH_RCCL_LIBRARY': fake, 'XH_FAKE_RCCL_DIR': str(tmp_path)})
        for k in ('RANK', 'WORLD_SIZE', 'XH_ROUTE_REASSOC'):
            env.pop(k, None)
        r = subprocess.run([sys.executable, str(script), ROOT, ini, str(n)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0 and 'PARENT_OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        if n > 1:
            assert r.stdout.count('of 900 cells on this rank') == 2
        outs[tag] = os.path.join(root, 'output', 'pm_abcd_mrtm_synth')
    for sc in SCALES:
        fn = diagnostics.FILE.format(sc)
        one, two = (open(os.path.join(outs[t], fn)).read() for t in ('one', 'two'))
        assert one == two and len(one.splitlines()) > 2, fn


# ---------------------------------------------------------------------------------------------- full size
def test_fullsize_against_numpy(tmp_path):
    ncell, nm = 67420, 720
    rng = np.random.default_rng(720)
    q = rng.lognormal(1.0, 1.2, (ncell, nm))
    q[rng.choice(ncell, 50, replace=False), rng.integers(0, nm, 50)] = np.nan
    ref = SimpleNamespace(area=rng.uniform(100.0, 3000.0, ncell), vic=rng.lognormal(-3.0, 1.0, (ncell, 30)),
                          unh=rng.lognormal(-3.0, 1.0, ncell),
                          wbmd=np.stack([np.arange(1, ncell + 1), rng.lognormal(-3.0, 1.0, ncell)], axis=1),
                          wbmc=np.stack([np.arange(ncell, 0, -1), rng.lognormal(-3.0, 1.0, ncell)], axis=1),
                          basin_ids=rng.integers(0, 236, ncell), country_ids=rng.integers(0, 250, ncell),
                          region_ids=rng.integers(0, 33, ncell),
                          basin_names=np.array(['Basin {}'.format(k) for k in range(1, 236)]),
                          country_names=np.array(['Country {}'.format(k) for k in range(249)]),
                          region_names=np.array(['Region {}'.format(k) for k in range(1, 33)]))
    s = SimpleNamespace(PerformDiagnostics=1, CreateTimeSeriesPlot=1, OutputFolder=str(tmp_path), StartYear=1951,
                        EndYear=2010, DiagnosticScale=0, TimeSeriesScale=1, TimeSeriesMapID=[0, 1], OutputInYear=0,
                        OutputUnit=0, device=0)
    ctx = _hip.get_context(0)
    d_q = ctx.upload(q)
    diagnostics.Diagnostics(s, d_q, ref)
    ac = q * 3.0
    tables = time_series.TimeSeriesPlot(s, d_q, ac, ref)
    d_q.free()
    want = D.diag_tables(q, 60, ref)
    for sc in SCALES:
        assert open(os.path.join(str(tmp_path), diagnostics.FILE.format(sc))).read() == _csv_text(want[sc]), sc
    qt, act, _ = tables['Basin']
    assert np.array_equal(qt, time_series.with_global(D.aggregation(ref.basin_ids, q)))
    assert np.array_equal(act, time_series.with_global(D.aggregation(ref.basin_ids, ac)))
    pngs = sorted(os.listdir(os.path.join(str(tmp_path), 'TimeSeriesPlot', 'Basin')))
    assert pngs == ['Basin0_Global_runoff.png', 'Basin0_Global_streamflow.png', 'Basin1_Basin 1_runoff.png',
                    'Basin1_Basin 1_streamflow.png']
