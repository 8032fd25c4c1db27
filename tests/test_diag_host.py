"""CPU tests of the diagnostics and time-series post-processors: parsing, refusals, the numpy / pandas restatements of
tests/diag_np.py against the reference's golden vectors (bit for bit), and the C-ABI entries."""
import io
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_np as D  # noqa: E402

from xanthos_amd import _hip, synth  # noqa: E402
from xanthos_amd.diagnostics import time_series  # noqa: E402
from xanthos_amd.diagnostics.diagnostics import scatter_table  # noqa: E402
from xanthos_amd.ini_reader import ConfigReader, ValidationException  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
LENGTHS = (1, 7, 8, 9, 127, 128, 129, 136, 300)


def _ini(tmp_path, **kw):
    w = synth.make_world(nrow=36, ncol=72, ncell=120, n_basins=4, seed=2)
    f = synth.hgm_forcing(w, synth.make_forcing(w, 24, nan_precip=False))
    root = str(tmp_path)
    ini = synth.write_hgm_example(root, w, f, 1971, 1972, runoff_spinup=12, routing_spinup=6)
    synth.write_diag_inputs(root, w)
    return synth.enable_diagnostics(ini, **kw), w


# ---------------------------------------------------------------------------------------------- parsing
def test_reader_parses_both_sections(tmp_path):
    ini, _ = _ini(tmp_path, diag_scale=2, plot_scale=3, map_id=7)
    s = ConfigReader(ini)
    assert s.PerformDiagnostics == 1 and s.CreateTimeSeriesPlot == 1
    assert s.DiagDir == os.path.join(s.InputFolder, 'diagnostics')
    assert s.VICDataFile == os.path.join(s.DiagDir, 'vic.csv') and s.WBMCDataFile == os.path.join(s.DiagDir, 'wbmc.csv')
    assert s.DiagnosticScale == 2 and s.TimeSeriesScale == 3 and s.TimeSeriesMapID == 7


def test_reader_parses_map_id_list(tmp_path):
    ini, _ = _ini(tmp_path, map_id=[0, 2, 5])
    assert ConfigReader(ini).TimeSeriesMapID == [0, 2, 5]


@pytest.mark.parametrize('flag,section', [('PerformDiagnostics', 'Diagnostics'), ('CreateTimeSeriesPlot', 'TimeSeriesPlot')])
def test_a_switch_without_its_section_is_refused_by_name(tmp_path, flag, section):
    ini, _ = _ini(tmp_path)
    text = open(ini).read()
    text = re.sub(r'\n\[{}\][^\[]*'.format(section), '\n', text)
    open(ini, 'w').write(text)
    with pytest.raises(ValidationException, match=flag):
        ConfigReader(ini)


def test_diagnostics_without_diag_dir_is_refused_by_name(tmp_path):
    ini, _ = _ini(tmp_path)
    text = open(ini).read().replace('DiagDir = diagnostics\n', '')
    open(ini, 'w').write(text)
    with pytest.raises(ValidationException, match='PerformDiagnostics.*DiagDir'):
        ConfigReader(ini)


def test_map_id_that_is_not_an_integer_is_refused(tmp_path):
    ini, _ = _ini(tmp_path)
    text = open(ini).read().replace('MapID = 999', 'MapID = all')
    open(ini, 'w').write(text)
    with pytest.raises(ValidationException, match='MapID'):
        ConfigReader(ini)


def test_plot_rows_follow_map_id_and_refuse_rows_beyond_the_table():
    assert time_series.plot_rows(999, 5, 6, 'Basin') == [0, 1, 2, 3, 4]
    assert time_series.plot_rows(3, 5, 6, 'Basin') == [3]
    assert time_series.plot_rows([0, 4], 5, 6, 'Basin') == [0, 4]
    with pytest.raises(ValidationException, match='MapID 5 is beyond the Basin table'):
        time_series.plot_rows(5, 5, 6, 'Basin')
    with pytest.raises(ValidationException, match='MapID 9'):
        time_series.plot_rows([1, 9], 5, 6, 'Country')
    with pytest.raises(ValidationException, match='MapID 4.*names'):
        time_series.plot_rows(999, 5, 4, 'GCAMRegion')


def test_scatter_table_keeps_the_reference_row_order():
    t = np.array([[2, 1.0], [3, 2.0], [2, 5.0], [0, 7.0]])
    assert np.array_equal(scatter_table(t, 4, 'WBM'), [0.0, 5.0, 2.0, 7.0])     # later rows win, id 0 -> last cell
    with pytest.raises(ValidationException, match='WBM: cell id 9'):
        scatter_table(np.array([[9, 1.0]]), 4, 'WBM')


# ---------------------------------------------------------------------------------------------- orders vs the golden
def _kernel_ref(g):
    return SimpleNamespace(**{k: g['k_' + k] for k in ('area', 'basin_ids', 'country_ids', 'region_ids', 'vic', 'unh',
                                                      'wbmd', 'wbmc', 'basin_names', 'country_names', 'region_names')})


def _csv_text(df):
    buf = io.StringIO()
    df.to_csv(buf, na_rep=0, index=False)
    return buf.getvalue()


@pytest.mark.parametrize('n', LENGTHS)
def test_diag_np_writes_the_reference_csvs(golden, n):
    g = golden('diag')
    y0, y1 = g['k{}_years'.format(n)]
    tables = D.diag_tables(np.ascontiguousarray(g['k_q'][:, :n]), int(y1 - y0 + 1), _kernel_ref(g))
    for sc in ('Basin', 'Country', 'Region'):
        assert _csv_text(tables[sc]) == str(g['k{}_{}_csv'.format(n, sc)]), sc


def test_pairwise_restatement_is_numpy_sum():
    rng = np.random.default_rng(3)
    for n in (1, 5, 7, 8, 9, 127, 128, 129, 136, 255, 256, 600, 720, 1201, 8192, 8193, 20000):
        a = rng.standard_normal((17, n)) * 10.0 ** rng.integers(-8, 8, (17, n))
        assert np.array_equal(D.pairwise_rows(a), np.sum(a, axis=1)), n


def test_kahan_restatement_is_pandas_groupby_sum():
    rng = np.random.default_rng(5)
    n = 3000
    v = rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-10, 17, (n, 3))
    v[rng.random((n, 3)) < 0.02] = np.nan
    v[11, 0], v[40, 1], v[41, 1], v[77, 2] = np.inf, np.inf, -np.inf, -np.inf
    ids = rng.integers(-2, 9, n)
    uniq, s, counts = D.kahan_groups(v, ids)
    df = pd.DataFrame(v, columns=['a', 'b', 'c'])
    df['id'] = ids
    want = df.groupby('id').sum()
    assert np.array_equal(uniq, want.index.values) and np.array_equal(counts, np.bincount(ids + 2)[uniq + 2])
    assert np.array_equal(s, want.values, equal_nan=True)
    big = pd.DataFrame({'x': [1e16, 1.0, 1.0], 'id': 0}).groupby('id').sum().values[0, 0]
    assert big == 1.0000000000000002e16 and D.kahan_groups(np.array([1e16, 1.0, 1.0]), [0, 0, 0])[1][0, 0] == big


def test_aggregation_restatement_is_the_reference_table(golden):
    g = golden('diag')
    assert np.array_equal(D.aggregation(g['ts_basin_ids'], g['ts_q']), g['ts_basin_table'])
    assert np.array_equal(D.aggregation(g['ts_country_ids'], g['ts_q']), g['ts_country_table'])


# ---------------------------------------------------------------------------------------------- C-ABI
def test_new_entries_in_header_and_signatures():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    for name in ('xh_diag_cell_total', 'xh_diag_group_sum'):
        assert re.search(r'\bint {}\('.format(name), header), name
        assert name in _hip.SIGNATURES, name
    assert _hip.ABI_VERSION == 7
    assert 'xh_diag.hip' in open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'Makefile')).read()
