"""Generate the hydropower golden vectors in this directory from the REAL reference (JGCRI/xanthos v2.4.1).

Run in the build container only (needs the reference checkout, which the GPU box does not have):

    python tests/golden/make_golden_hydro.py

The reference modules are imported unmodified by file path, as make_golden_pet_ext.py imports its modules.
``HydropowerActual`` runs as it is.  ``HydropowerPotential`` indexes a Series as ``s[:, np.newaxis]``
(potential.py:36), which pandas >= 2.0 refuses with a ValueError; so the name ``pd`` of the LOADED module (not the file)
is bound to a thin wrapper of pandas whose ``read_csv`` returns a DataFrame whose columns answer tuple indexing with
their numpy array -- the behaviour of the pandas the reference was written against.  Everything else is pandas itself.

  hydro.npz  pot_*   HydropowerPotential on 400 cells x 84 months starting in April (partial first and last years), NaN
                     cells, zero elevations: q, gridData, both csv texts, constrain_q per cell, and the per-cell annual
                     energies (the reference run again with one region per cell: its technical csv is E)
             act_*   HydropowerActual on a 300-cell world x 96 months starting in July with 60 dams (idxmin ties on cell
                     borders, CAPLIVE / HEAD fall-backs, NaN rule curves): the input tree (zip), q, power_all_dams,
                     grid_ids, dr_ar_assumed, q_Mm3, the last dam's env_flow and the csv text
             model_* the reference's ConfigRunner on a small hargreaves_gwam_mrtm tree with both switches on: the tree
                     (zip) and the three csv texts
"""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
import pandas as pd

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _TupleSeries(pd.Series):
    """A Series that answers ``s[:, np.newaxis]`` with its array, as pandas < 2.0 did."""

    @property
    def _constructor(self):
        return _TupleSeries

    def __getitem__(self, key):
        if isinstance(key, tuple):
            return self.values[key]
        return super().__getitem__(key)


class _Frame(pd.DataFrame):
    _constructor_sliced = _TupleSeries

    @property
    def _constructor(self):
        return _Frame


def _pandas_wrapper():
    w = types.ModuleType('pandas_tuple_columns')
    w.__dict__.update({k: v for k, v in pd.__dict__.items() if not k.startswith('__')})
    w.read_csv = lambda *a, **k: _Frame(pd.read_csv(*a, **k))
    return w


ref_pot = _load('ref_pot', 'xanthos/hydropower/potential.py')
ref_pot.pd = _pandas_wrapper()
ref_act = _load('ref_act', 'xanthos/hydropower/actual.py')

import make_golden_hgm as hgm  # noqa: E402  (stubs configobj, imports the reference's ConfigRunner)
from xanthos_amd import synth  # noqa: E402

sys.modules['xanthos.hydropower.potential'].pd = ref_pot.pd     # the package's copy, which the reference's components call


def _text(path):
    return np.array(open(path).read())


def _zip(root, sub):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:
        for d, _, files in os.walk(os.path.join(root, sub)):
            for fn in files:
                full = os.path.join(d, fn)
                z.write(full, os.path.relpath(full, root))
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def golden_potential(out):
    rng = np.random.default_rng(2017)
    nc, nm = 400, 84
    q = rng.lognormal(3.0, 1.5, (nc, nm))
    q[rng.random(nc) < 0.05, :] *= 0.0                       # dry cells
    q[rng.random(q.shape) < 0.002] = np.nan                 # NaN months: the whole cell becomes NaN
    q[7, 3] = -1.0                                           # a negative flow: clipped to 0
    q[9, :] = 5.0                                            # ties everywhere
    grid = pd.DataFrame({'ID': np.arange(1, nc + 1), 'long': np.zeros(nc), 'lati': np.zeros(nc),
                         'elevD': np.round(rng.uniform(0, 300, nc), 3), 'regID': rng.integers(0, 33, nc),
                         'inGrandELEC': (rng.random(nc) < 0.6).astype(int)})
    grid.loc[rng.random(nc) < 0.05, 'elevD'] = 0.0
    q_ex, ef, start = 0.75, 0.9, '4/1971'
    with tempfile.TemporaryDirectory() as d:
        s = types.SimpleNamespace(GridData=os.path.join(d, 'gridData.csv'), q_ex=q_ex, ef=ef, hpot_start_date=start,
                                  OutputFolder=d, ProjectName='pot')
        grid.to_csv(s.GridData, index=False)
        ref_pot.HydropowerPotential(s, q.copy())
        out['pot_techpot_csv'] = _text(os.path.join(d, 'tech_hydro_pot_by_gcam_region_EJperyr_pot.csv'))
        out['pot_expl_csv'] = _text(os.path.join(d, 'tech_expliot_hyd_pot_by_gcam_region_EJperyr_pot.csv'))
        g1 = grid.copy()
        g1['regID'] = np.arange(nc)                          # one region per cell: the technical csv is E per cell
        g1.to_csv(s.GridData, index=False)
        ref_pot.HydropowerPotential(s, q.copy())
        e = pd.read_csv(os.path.join(d, 'tech_hydro_pot_by_gcam_region_EJperyr_pot.csv'), float_precision='round_trip')
    out['pot_E'] = e.iloc[:, 1:].values
    out['pot_years'] = np.array([int(c) for c in e.columns[1:]])
    out['pot_constrained'] = np.stack([ref_pot.constrain_q(q[c], q_ex) for c in range(nc)])
    out.update(pot_q=q, pot_elevD=grid['elevD'].values, pot_regID=grid['regID'].values,
               pot_inGrandELEC=grid['inGrandELEC'].values, pot_q_ex=q_ex, pot_ef=ef, pot_start=np.array(start))
    print('potential: NaN cells', int(np.isnan(q).any(axis=1).sum()), 'E', out['pot_E'].shape)


def golden_actual(out):
    w = synth.make_world(nrow=360, ncol=720, ncell=300, n_basins=3, seed=4)
    rng = np.random.default_rng(1593)
    nm, start = 96, '7/1971'
    q = rng.lognormal(4.0, 1.0, (w.ncell, nm))
    q[:, 20:26] *= 0.01                                      # a dry half-year: reservoirs draw down
    with tempfile.TemporaryDirectory() as root:
        hyd = synth.write_hydro_inputs(root, w, ndams=60, seed=12)
        s = types.SimpleNamespace(HydroDamData=os.path.join(hyd, 'resData_1593.csv'),
                                  GridData=os.path.join(hyd, 'gridData.csv'),
                                  DrainArea=os.path.join(hyd, 'DRT_half_SourceArea_globe_float.txt'),
                                  MissingCap=os.path.join(hyd, 'simulated_cap_by_country.csv'),
                                  rule_curves=os.path.join(hyd, 'rule_curves_1593.npy'), ProjectName='act',
                                  OutputFolder=root, hact_start_date=start)
        a = ref_act.HydropowerActual(s, q.copy())
        out['act_csv'] = _text(os.path.join(root, 'actual_hydro_by_gcam_region_EJperyr_act.csv'))
        out['act_tree_zip'] = _zip(root, 'input')
    out.update(act_q=q, act_start=np.array(start), act_power=a.power_all_dams, act_grid_ids=np.asarray(a.grid_ids),
               act_dr_ar_assumed=a.dr_ar_assumed, act_q_Mm3=a.q_Mm3, act_env_flow_last=np.asarray(a.env_flow))
    print('actual: dams', a.power_all_dams.shape, 'zero power', int((a.power_all_dams == 0).sum()))


def golden_model(out):
    w = synth.make_world(nrow=360, ncol=720, ncell=150, n_basins=4, seed=3)
    y0, y1 = 1971, 1972
    f = synth.hgm_forcing(w, synth.make_forcing(w, 24, nan_precip=False))
    with tempfile.TemporaryDirectory() as root:
        ini = synth.write_hgm_example(root, w, f, y0, y1, runoff_spinup=12, routing_spinup=6, output_vars=('q',))
        synth.write_hydro_inputs(root, w, ndams=25, seed=13)
        synth.enable_hydro(ini, hpot_start_date='3/1971', hact_start_date='1/1971', q_ex=0.8, ef=0.87)
        res = hgm._tree_case('model', root, ini, w)
        od = os.path.join(root, 'output', 'hargreaves_gwam_mrtm_synth')
        for key, name in (('techpot', 'tech_hydro_pot_by_gcam_region_EJperyr_'),
                          ('expl', 'tech_expliot_hyd_pot_by_gcam_region_EJperyr_'),
                          ('actual', 'actual_hydro_by_gcam_region_EJperyr_')):
            out['model_{}_csv'.format(key)] = _text(os.path.join(od, name + 'hargreaves_gwam_mrtm_synth.csv'))
    for k in ('model_tree_zip', 'model_old_root', 'model_ini_name', 'model_Avg_ChFlow'):
        out[k] = res[k]
    print('model: Avg_ChFlow', res['model_Avg_ChFlow'].shape)


if __name__ == '__main__':
    import warnings
    warnings.simplefilter('ignore')
    out = {}
    golden_potential(out)
    golden_actual(out)
    golden_model(out)
    np.savez_compressed(os.path.join(HERE, 'hydro.npz'), **out)
    print('hydro.npz', os.path.getsize(os.path.join(HERE, 'hydro.npz')), 'bytes')
