"""Host-side tests of the hydropower post-processors: configuration, the dam lookups, the summation orders the kernels
restate (numpy restatements against the reference's golden vectors, bit for bit) and the host-built csv files."""
import io
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hydro_np as H  # noqa: E402

from xanthos_amd import synth  # noqa: E402
from xanthos_amd.drought.drought_stats import quantile_plan  # noqa: E402
from xanthos_amd.hydropower import actual, potential  # noqa: E402
from xanthos_amd.ini_reader import ConfigReader, ValidationException  # noqa: E402


def _act_tree(golden, tmp_path):
    g = golden('hydro')
    with zipfile.ZipFile(io.BytesIO(g['act_tree_zip'].tobytes())) as z:
        z.extractall(str(tmp_path))
    return g, os.path.join(str(tmp_path), 'input', 'hydropower')


# ---------------------------------------------------------------------------------------------- configuration
@pytest.fixture
def ini(tmp_path):
    w = synth.make_world(nrow=36, ncol=72, ncell=200, n_basins=3, seed=2)
    path = synth.write_example(str(tmp_path), w, synth.make_forcing(w, 24), 1971, 1972, runoff_spinup=12)
    synth.write_hydro_inputs(str(tmp_path), w, ndams=10)
    return path


def _edit(path, *pairs):
    text = open(path).read()
    for a, b in pairs:
        assert a in text, a
        text = text.replace(a, b, 1)
    open(path, 'w').write(text)
    return path


def test_hydropower_switches_are_accepted(ini):
    synth.enable_hydro(ini, hpot_start_date='3/1971', q_ex=0.8, ef=0.9)
    s = ConfigReader(ini)
    assert s.CalculateHydropowerPotential == 1 and s.CalculateHydropowerActual == 1
    assert (s.hpot_start_date, s.hact_start_date, s.q_ex, s.ef) == ('3/1971', '1/1971', 0.8, 0.9)
    assert s.GridData.endswith(os.path.join('hydropower', 'gridData.csv'))
    for attr in ('HydroDamData', 'MissingCap', 'rule_curves', 'DrainArea'):
        assert os.path.isfile(getattr(s, attr)), attr


def test_potential_alone_reads_hydactdir(ini):
    synth.enable_hydro(ini, actual=False)
    s = ConfigReader(ini)
    assert s.CalculateHydropowerPotential == 1 and os.path.isfile(s.GridData)
    assert not hasattr(s, 'hact_start_date')


@pytest.mark.parametrize('edit,match', [
    (('\n[HydropowerPotential]', '\n[NotPotential]'), r'no \[HydropowerPotential\] section'),
    (('\n[HydropowerActual]', '\n[NotActual]'), r'no \[HydropowerActual\] section'),
    (('HydActDir = hydropower\n', ''), 'needs HydActDir'),
    (('q_ex = 0.9', 'q_ex = 1.5'), r'must lie in \[0, 1\]'),
    (('q_ex = 0.9', 'q_ex = -0.1'), r'must lie in \[0, 1\]'),
    (('q_ex = 0.9\n', ''), 'q_ex is required'),
    (('hact_start_date = 1/1971', 'hact_start_date = 13/1971'), 'is not a month'),
    (('routing_module = mrtm', 'routing_module = none'), 'routing_module = mrtm'),
])
def test_hydropower_validation(ini, edit, match):
    synth.enable_hydro(ini)
    _edit(ini, edit)
    with pytest.raises(ValidationException, match=match):
        ConfigReader(ini)


def test_griddata_rows_must_match_cells(ini, tmp_path):
    synth.enable_hydro(ini)
    p = os.path.join(str(tmp_path), 'input', 'hydropower', 'gridData.csv')
    pd.read_csv(p).iloc[:-1].to_csv(p, index=False)
    with pytest.raises(ValidationException, match='matched to the 200 cells'):
        ConfigReader(ini)


@pytest.mark.parametrize('flag', ['PerformDiagnostics', 'CreateTimeSeriesPlot'])
def test_diagnostics_and_plots_stay_refused(ini, flag):
    _edit(ini, ('\n[PET]', '\n{} = 1\n[PET]'.format(flag)))
    with pytest.raises(ValidationException, match=flag):
        ConfigReader(ini)


# ---------------------------------------------------------------------------------------------- dam lookups
def test_grid_ids_and_drain_areas_match_reference(golden, tmp_path):
    g, hyd = _act_tree(golden, tmp_path)
    grid = pd.read_csv(os.path.join(hyd, 'gridData.csv'))
    res = pd.read_csv(os.path.join(hyd, 'resData_1593.csv'))
    loc = grid[['ID', 'long', 'lati']]
    ids = actual.find_grid_ids(loc, res)
    assert np.array_equal(ids, g['act_grid_ids'])
    area = actual.find_drain_areas(loc, ids, np.loadtxt(os.path.join(hyd, 'DRT_half_SourceArea_globe_float.txt')))
    assert np.array_equal(area, g['act_dr_ar_assumed'])
    # the tree holds dams exactly on a cell border (an idxmin tie between two longitudes)
    off = res['LONG_DD'].values - grid['long'].values[ids - 1]
    assert (off == 0.25).sum() >= 3


def test_grid_id_ties_take_the_first_row_in_griddata_order():
    # longitudes 1.0 and 2.0 are equally near 1.5: idxmin takes the one of the earlier row -- 2.0 here (row 0)
    loc = pd.DataFrame({'ID': [1, 2, 3, 4], 'long': [2.0, 1.0, 2.0, 1.0], 'lati': [5.0, 5.0, 6.0, 6.0]})
    res = pd.DataFrame({'LONG_DD': [1.5, 1.5, 1.2], 'LAT_DD': [5.5, 5.2, 5.9]})
    # latitude 5.5: 5.0 (row 0) before 6.0 (row 2) -> (2.0, 5.0) = ID 1; 5.2 -> 5.0 -> ID 1; (1.0, 6.0) = ID 4
    assert actual.find_grid_ids(loc, res).tolist() == [1, 1, 4]
    # the unique land latitudes, descending: 6.0 is row 0, 5.0 row 1; the longitudes ascending: 1.0 col 0, 2.0 col 1
    area = np.arange(4.0).reshape(2, 2)
    assert actual.find_drain_areas(loc, np.array([1, 4]), area).tolist() == [3.0, 0.0]


def test_grid_id_refuses_zero_or_several_rows():
    loc = pd.DataFrame({'ID': [1, 2], 'long': [1.0, 2.0], 'lati': [5.0, 6.0]})
    with pytest.raises(ValueError, match='dam 0 .* 0 gridData rows'):
        actual.find_grid_ids(loc, pd.DataFrame({'LONG_DD': [1.1], 'LAT_DD': [5.9]}))
    loc2 = pd.DataFrame({'ID': [1, 2], 'long': [1.0, 1.0], 'lati': [5.0, 5.0]})
    with pytest.raises(ValueError, match='2 gridData rows'):
        actual.find_grid_ids(loc2, pd.DataFrame({'LONG_DD': [1.0], 'LAT_DD': [5.0]}))


# ---------------------------------------------------------------------------------------------- summation orders
def test_env_flow_restatement_is_bit_exact(golden, tmp_path):
    g, hyd = _act_tree(golden, tmp_path)
    res = pd.read_csv(os.path.join(hyd, 'resData_1593.csv'))
    inflow = ((g['act_q'][g['act_grid_ids'] - 1].T * res['CATCH'].values) / g['act_dr_ar_assumed']) * H.MM3
    assert np.array_equal(inflow, g['act_q_Mm3'])
    env = H.env_flow(inflow, str(g['act_start']))
    assert np.array_equal(env[-1], g['act_env_flow_last'])
    power = H.march(inflow, env, np.load(os.path.join(hyd, 'rule_curves_1593.npy')), H.dam_parameters(res),
                    str(g['act_start']))
    assert np.array_equal(power, g['act_power'])


def test_pairwise_and_compensated_sums_follow_numpy_and_pandas():
    x = np.array([1.0] + [1e-16] * 11)
    s, n = H.kahan_rows(x[:, None], np.zeros(12, dtype=int), 1)
    assert s[0, 0] == pd.Series(x).groupby(np.zeros(12)).sum().iloc[0] and s[0, 0] != np.cumsum(x)[-1]
    rng = np.random.default_rng(3)
    for n in (1, 7, 8, 129, 600, 1031):
        a = rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-3, 12, (n, 3))
        assert np.array_equal(H.pairwise_sum(a), [np.sum(a[:, j]) for j in range(3)])
        assert H.pairwise_sum(a)[0] / n == pd.DataFrame(a)[0].mean()


@pytest.mark.parametrize('n', [600, 1200])
@pytest.mark.parametrize('q', [0.0, 0.1, 0.5, 0.75, 0.9, 0.95, 0.999, 1.0])
def test_quantile_plan_matches_percentile(n, q):
    rng = np.random.default_rng(n)
    x = rng.lognormal(2.0, 1.0, n)
    x[::7] = x[3]                                                   # ties
    k_prev, k_next, gamma = quantile_plan(n, (q * 100) / 100.0)
    srt = np.sort(x)
    a, b = srt[k_prev], srt[k_next]
    r = a + (b - a) * gamma
    if gamma >= 0.5:
        r = b - (b - a) * (1 - gamma)
    assert r == np.percentile(x, q * 100)


def test_potential_restatement_is_bit_exact(golden):
    g = golden('hydro')
    q_max, E = H.potential_cells(g['pot_q'], g['pot_elevD'], float(g['pot_q_ex']), float(g['pot_ef']), str(g['pot_start']))
    assert np.array_equal(E, g['pot_E'])
    assert np.array_equal(np.clip(g['pot_q'], 0, q_max[:, None]), g['pot_constrained'], equal_nan=True)


# ---------------------------------------------------------------------------------------------- host-built csv files
def test_potential_tables_write_the_reference_text(golden, tmp_path):
    g = golden('hydro')
    E = g['pot_E']
    reg, inge = g['pot_regID'], g['pot_inGrandELEC']
    _, years = potential.year_plan(str(g['pot_start']), g['pot_q'].shape[1])
    assert [int(str(y)) for y in years] == g['pot_years'].tolist()
    res = SimpleNamespace(years=years, groups=[H.region_sums(E, reg), H.region_sums(E, reg * inge)])
    techpot, expl = potential.region_tables(res)
    potential.write_tables(techpot, expl, str(tmp_path), 'pot')
    assert open(str(tmp_path / potential.TECHPOT_FILE.format('pot'))).read() == str(g['pot_techpot_csv'])
    assert open(str(tmp_path / potential.EXPL_FILE.format('pot'))).read() == str(g['pot_expl_csv'])


def _actual_host(hyd, g, out_dir):
    a = actual.HydropowerActual.__new__(actual.HydropowerActual)
    a.res_data = pd.read_csv(os.path.join(hyd, 'resData_1593.csv'))
    a.missing_cap = pd.read_csv(os.path.join(hyd, 'simulated_cap_by_country.csv'))
    _, a.years = potential.year_plan(str(g['act_start']), g['act_power'].shape[0])
    a.annual_power = H.annual_means(g['act_power'], str(g['act_start']))
    a.filename_hydro = os.path.join(out_dir, actual.HYDRO_FILE.format('act'))
    return a


def test_actual_region_table_writes_the_reference_text(golden, tmp_path):
    g, hyd = _act_tree(golden, tmp_path / 'tree')
    a = _actual_host(hyd, g, str(tmp_path))
    a.to_region()
    a.write_output()
    assert open(a.filename_hydro).read() == str(g['act_csv'])


def test_actual_refuses_a_country_table_of_another_length(golden, tmp_path):
    g, hyd = _act_tree(golden, tmp_path / 'tree')
    a = _actual_host(hyd, g, str(tmp_path))
    a.missing_cap = a.missing_cap.iloc[:-1]
    with pytest.raises(ValueError, match='factor values for the 7 countries'):
        a.to_region()


def test_a_library_without_the_new_symbols_asks_for_a_rebuild(tmp_path):
    """A library built before the hydropower entries (same ABI version, symbols missing) is refused with HipUnavailable."""
    import subprocess
    src = tmp_path / 'stale.c'
    src.write_text('int xh_abi_version(void) { return 7; }\n')
    so = str(tmp_path / 'libstale.so')
    subprocess.run(['cc', '-shared', '-fPIC', '-o', so, str(src)], check=True)
    code = ('import sys; sys.path.insert(0, {!r})\nfrom xanthos_amd import _hip\ntry:\n    _hip.lib()\n'
            'except _hip.HipUnavailable as e:\n    print("REFUSED", e)\n').format(
        os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, XH_LIBRARY=so), capture_output=True, text=True,
                         timeout=120)
    assert 'REFUSED' in out.stdout and 'lacks xh_' in out.stdout and 'rebuild' in out.stdout, out.stdout + out.stderr
