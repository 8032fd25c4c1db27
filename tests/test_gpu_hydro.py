"""GPU tests of the hydropower post-processors (csrc/xh_hydro.hip) against the reference's golden vectors, whole model runs
(one rank and two) and, at full size, the numpy restatements of tests/hydro_np.py."""
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
import hydro_np as H  # noqa: E402

from xanthos_amd import _hip, synth  # noqa: E402
from xanthos_amd.hydropower import actual, potential  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
FAKE = os.path.join(ROOT, 'tests', 'fake_rccl')


def _pot_settings(g, d, regid=None):
    grid = pd.DataFrame({'ID': np.arange(1, len(g['pot_elevD']) + 1), 'long': 0.0, 'lati': 0.0, 'elevD': g['pot_elevD'],
                         'regID': g['pot_regID'] if regid is None else regid, 'inGrandELEC': g['pot_inGrandELEC']})
    s = SimpleNamespace(GridData=os.path.join(d, 'gridData.csv'), q_ex=float(g['pot_q_ex']), ef=float(g['pot_ef']),
                        hpot_start_date=str(g['pot_start']), OutputFolder=d, ProjectName='pot', device=0)
    grid.to_csv(s.GridData, index=False)
    return s


def _act_settings(g, d):
    with zipfile.ZipFile(io.BytesIO(g['act_tree_zip'].tobytes())) as z:
        z.extractall(d)
    hyd = os.path.join(d, 'input', 'hydropower')
    return SimpleNamespace(HydroDamData=os.path.join(hyd, 'resData_1593.csv'), GridData=os.path.join(hyd, 'gridData.csv'),
                           DrainArea=os.path.join(hyd, 'DRT_half_SourceArea_globe_float.txt'),
                           MissingCap=os.path.join(hyd, 'simulated_cap_by_country.csv'),
                           rule_curves=os.path.join(hyd, 'rule_curves_1593.npy'), ProjectName='act', OutputFolder=d,
                           hact_start_date=str(g['act_start']), device=0)


# ---------------------------------------------------------------------------------------------- potential
def test_qmax_and_annual_energy_are_bit_exact(golden, tmp_path):
    g = golden('hydro')
    q = g['pot_q']
    res = potential.HydropowerPotential(_pot_settings(g, str(tmp_path)), q)
    q_max = np.percentile(q, float(g['pot_q_ex']) * 100, axis=1)
    assert np.array_equal(res.q_max, q_max, equal_nan=True) and np.isnan(res.q_max).sum() > 10
    assert np.array_equal(res.E, g['pot_E'])
    assert (res.E[np.isnan(q).any(axis=1)] == 0).all()                  # a NaN month zeroes the whole cell
    assert np.array_equal(potential.constrain_q(q, float(g['pot_q_ex'])), g['pot_constrained'], equal_nan=True)
    for c in (5, int(np.nonzero(~np.isnan(q).any(axis=1))[0][0])):          # one series: a NaN cell, a finite one
        assert np.array_equal(potential.constrain_q(q[c], float(g['pot_q_ex'])), g['pot_constrained'][c], equal_nan=True)


def test_potential_csvs_equal_the_reference_text(golden, tmp_path):
    g = golden('hydro')
    s = _pot_settings(g, str(tmp_path))
    ctx = _hip.get_context(0)
    d_q = ctx.upload(g['pot_q'])                                        # a DeviceArray is used in place
    potential.HydropowerPotential(s, d_q)
    d_q.free()
    assert open(os.path.join(str(tmp_path), potential.TECHPOT_FILE.format('pot'))).read() == str(g['pot_techpot_csv'])
    assert open(os.path.join(str(tmp_path), potential.EXPL_FILE.format('pot'))).read() == str(g['pot_expl_csv'])


@pytest.mark.parametrize('nmonths', [12, 601, 4096])
def test_qmax_kernel_order_statistics(nmonths):
    rng = np.random.default_rng(nmonths)
    q = rng.lognormal(1.0, 2.0, (300, nmonths))
    q[::3] = np.round(q[::3])                                           # many ties
    q[1] = -q[1]
    q[2, :] = 0.0
    q[4, 5] = np.inf
    ctx = _hip.get_context(0)
    d_q = ctx.upload(q)
    for ex in (0.0, 0.37, 0.5, 0.9, 1.0):
        d = potential.qmax_device(ctx, d_q, ex)
        assert np.array_equal(d.download(), np.percentile(q, ex * 100, axis=1), equal_nan=True), ex
        d.free()
    d_q.free()


# ---------------------------------------------------------------------------------------------- actual
def test_actual_is_bit_exact(golden, tmp_path):
    g = golden('hydro')
    s = _act_settings(g, str(tmp_path))
    a = actual.HydropowerActual(s, g['act_q'])
    assert np.array_equal(a.grid_ids, g['act_grid_ids'])
    assert np.array_equal(a.dr_ar_assumed, g['act_dr_ar_assumed'])
    assert np.array_equal(a.env_flow[-1], g['act_env_flow_last'])
    assert np.array_equal(a.power_all_dams, g['act_power'])
    assert np.array_equal(a.annual_power, H.annual_means(g['act_power'], str(g['act_start'])))
    assert open(a.filename_hydro).read() == str(g['act_csv'])


def test_actual_refuses_a_nan_dam(golden, tmp_path):
    g = golden('hydro')
    q = g['act_q'].copy()
    q[g['act_grid_ids'][4] - 1, 30] = np.nan
    with pytest.raises(ValueError, match='dam 4 .* holds NaN'):
        actual.HydropowerActual(_act_settings(g, str(tmp_path)), q)


def test_actual_refuses_a_month_without_rule_curve_row(golden, tmp_path):
    g = golden('hydro')
    s = _act_settings(g, str(tmp_path))
    rc = np.load(s.rule_curves)
    rc[:, 5, 9] = 2.0                                                   # June: every row above any storage fraction
    np.save(s.rule_curves, rc)
    with pytest.raises(ValueError, match=r'dam 9 \(.*\): in month 11 of the run no rule-curve row'):
        actual.HydropowerActual(s, g['act_q'])


# ---------------------------------------------------------------------------------------------- whole model runs
def _csv_close(a_path, b_text, rtol):
    a = pd.read_csv(a_path)
    b = pd.read_csv(io.StringIO(b_text))
    assert list(a.columns) == list(b.columns) and a.shape == b.shape and (a['region'] == b['region']).all()
    x, y = a.iloc[:, 1:].values, b.iloc[:, 1:].values
    assert (np.abs(x - y) <= rtol * np.abs(y) + 1e-300).all(), float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))


def test_model_run_writes_the_reference_csvs(golden, tmp_path):
    from xanthos_amd.model import Xanthos
    g = golden('hydro')
    root = str(tmp_path)
    with zipfile.ZipFile(io.BytesIO(g['model_tree_zip'].tobytes())) as z:
        z.extractall(root)
    ini = os.path.join(root, str(g['model_ini_name']))
    text = open(ini).read().replace(str(g['model_old_root']), root)
    open(ini, 'w').write(text)
    c = Xanthos(ini).execute()
    assert c.pipe is not None and 'Avg_ChFlow' not in c._host           # the post-processors read it in HBM
    od = os.path.join(root, 'output', 'hargreaves_gwam_mrtm_synth')
    # the routed flow itself agrees with the reference's to rounding, so the csvs are compared as numbers
    for key, name in (('techpot', potential.TECHPOT_FILE), ('expl', potential.EXPL_FILE), ('actual', actual.HYDRO_FILE)):
        _csv_close(os.path.join(od, name.format('hargreaves_gwam_mrtm_synth')), str(g['model_{}_csv'.format(key)]), 1e-9)


RUN_MODEL_PARENT = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
from xanthos_amd import run_model
res = run_model(sys.argv[2], gpus=int(sys.argv[3]))
print('PARENT_OK')
'''


def test_two_ranks_write_the_same_hydropower_csvs(tmp_path):
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=33)
    f = synth.make_forcing(w, 36, nan_precip=False)
    fake = os.path.join(FAKE, 'librccl.so.1')
    if not os.path.isfile(fake):
        subprocess.run(['make', '-C', FAKE], check=True, capture_output=True)
    outs = {}
    for tag, n in (('one', 1), ('two', 2)):
        root = str(tmp_path / tag)
        os.makedirs(root)
        ini = synth.write_example(root, w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, output_vars=('q',))
        text = open(ini).read().replace('routing_spinup', 'routing_form = exact\n    routing_spinup', 1)
        open(ini, 'w').write(text)
        synth.write_hydro_inputs(root, w, ndams=30, seed=21)
        synth.enable_hydro(ini, hpot_start_date='5/1971', hact_start_date='1/1971')
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
    for name in (potential.TECHPOT_FILE, potential.EXPL_FILE, actual.HYDRO_FILE):
        fn = name.format('pm_abcd_mrtm_synth')
        one, two = (open(os.path.join(outs[t], fn)).read() for t in ('one', 'two'))
        assert one == two and len(one.splitlines()) > 1, fn


# ---------------------------------------------------------------------------------------------- full size
def test_fullsize_against_numpy(tmp_path):
    ncell, nm, ndams = 67420, 600, 1593
    rng = np.random.default_rng(67420)
    flat = np.sort(rng.choice(360 * 720, ncell, replace=False))
    rows, cols = flat % 360, flat // 360                                 # column-major: id grows with lon, then lat
    coords = np.stack([np.arange(1, ncell + 1), -180 + (cols + 0.5) * 0.5, -90 + (rows + 0.5) * 0.5], axis=1)
    world = SimpleNamespace(ncell=ncell, coords=coords)
    hyd = synth.write_hydro_inputs(str(tmp_path), world, ndams=ndams, seed=5)
    grid = pd.read_csv(os.path.join(hyd, 'gridData.csv'))
    res = pd.read_csv(os.path.join(hyd, 'resData_1593.csv'))
    ids = actual.find_grid_ids(grid[['ID', 'long', 'lati']], res)
    q = rng.lognormal(4.0, 1.2, (ncell, nm))
    nan_cells = np.setdiff1d(rng.choice(ncell, 80, replace=False), ids - 1)
    q[nan_cells, rng.integers(0, nm, len(nan_cells))] = np.nan
    ctx = _hip.get_context(0)
    d_q = ctx.upload(q)
    s = SimpleNamespace(GridData=os.path.join(hyd, 'gridData.csv'), q_ex=0.9, ef=0.85, hpot_start_date='10/1950',
                        HydroDamData=os.path.join(hyd, 'resData_1593.csv'),
                        DrainArea=os.path.join(hyd, 'DRT_half_SourceArea_globe_float.txt'),
                        MissingCap=os.path.join(hyd, 'simulated_cap_by_country.csv'),
                        rule_curves=os.path.join(hyd, 'rule_curves_1593.npy'), hact_start_date='1/1951',
                        OutputFolder=str(tmp_path / 'out'), ProjectName='full', device=0)
    p = potential.HydropowerPotential(s, d_q)
    a = actual.HydropowerActual(s, d_q)
    d_q.free()
    q_max, E = H.potential_cells(q, grid['elevD'].values, 0.9, 0.85, '10/1950')
    assert np.array_equal(p.q_max, q_max, equal_nan=True)
    assert np.array_equal(p.E, E)
    _, reg = H.region_sums(E, grid['regID'].values)
    assert np.array_equal(p.groups[0][1], reg)
    assert np.array_equal(a.grid_ids, ids)
    inflow = ((q[ids - 1].T * res['CATCH'].values) / a.dr_ar_assumed) * H.MM3
    env = H.env_flow(inflow, '1/1951')
    assert np.array_equal(a.env_flow, env)
    power = H.march(inflow, env, np.load(s.rule_curves), H.dam_parameters(res), '1/1951')
    assert np.array_equal(a.power_all_dams, power)
    assert np.array_equal(a.annual_power, H.annual_means(power, '1/1951'))
