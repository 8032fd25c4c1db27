"""Generate the Hargreaves / GWAM golden vectors in this directory from the REAL reference (JGCRI/xanthos v2.4.1).

Run in the build container only (needs the reference checkout, which the GPU box does not have):

    python tests/golden/make_golden_hgm.py

The reference is imported unmodified, the way make_golden.py imports it (hargreaves.py / gwam.py / general.py by file
path, the package with a stub for ``configobj``).  Each fixture stores the crafted inputs AND the reference's outputs;
fixtures are data only.

  hargreaves.npz  calc_sinusoidal_factor for 1971-1976 and calculate_pet month by month on 512 cells (latitudes from pole
                  to pole: polar night and polar day, both arccos clamps, the equator) with negative / NaN / inf DTR and
                  NaN / +-inf temperature, prepared as the loader and prep_arrays / prep_pet prepare them
  gwam.npz        the reference driver's month loop (spin-up pass, then simulation; one precipitation column per pass)
                  on 512 cells x 36 months with every branch of runoffgen, plus the same loop with month m's precipitation
  hgm.npz         the reference's ConfigRunner on small hargreaves_gwam_mrtm trees on the 360 x 720 geometry (historic,
                  future mode) and one hargreaves_abcd_mrtm tree, settings from this package's ConfigReader; the trees
                  as zips
"""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_hg = _load('ref_hg', 'xanthos/pet/hargreaves.py')
ref_gwam = _load('ref_gwam', 'xanthos/runoff/gwam.py')
ref_general = _load('ref_general', 'xanthos/utils/general.py')

stub = types.ModuleType('configobj')
stub.ConfigObj = dict
sys.modules['configobj'] = stub
sys.path.insert(0, REF)
import matplotlib  # noqa: E402
matplotlib.use('Agg')
from xanthos.configurations import ConfigRunner as RefRunner  # noqa: E402

from xanthos_amd import synth  # noqa: E402
from xanthos_amd.ini_reader import ConfigReader  # noqa: E402

NC = 512


def golden_hargreaves():
    rng = np.random.default_rng(1971)
    y0, y1 = 1971, 1976
    tab = ref_general.set_month_arrays(72, y0, y1)
    dec, dr = ref_general.calc_sinusoidal_factor(tab)
    lat_deg = np.concatenate([[90.0, -90.0, 0.0, 89.5, -89.5, 66.6, -66.6, 70.0, -70.0, 23.4],
                              rng.uniform(-90, 90, NC - 10)])
    lat = np.radians(lat_deg)
    temp = rng.uniform(-30, 40, (NC, 72))
    dtr = rng.uniform(-3, 18, (NC, 72))
    temp[rng.random(temp.shape) < 0.02] = np.nan
    dtr[rng.random(dtr.shape) < 0.02] = np.nan
    temp[3, 4], temp[4, 5], dtr[5, 6], dtr[6, 7], dtr[7, 8] = np.inf, -np.inf, np.inf, -np.inf, -0.5
    # the loader (data_load.py:83-84) zeroes negative DTR, prep_arrays / prep_pet (components.py:144-187) nan_to_num both
    d_load = dtr.copy()
    d_load[np.where(d_load < 0)] = 0
    pet = np.zeros((NC, 72))
    for nm in range(72):
        T = np.nan_to_num(np.nan_to_num(temp[:, nm]))
        D = np.nan_to_num(np.nan_to_num(d_load[:, nm]))
        pet[:, nm] = ref_hg.calculate_pet(T, D, lat, np.copy(dec[nm]), np.copy(dr[nm]), np.copy(tab[nm, 2]))
    np.savez_compressed(os.path.join(HERE, 'hargreaves.npz'), start_year=y0, end_year=y1, yr_imth_ndays=tab,
                        solar_dec=dec, dr=dr, lat=lat, temp=temp, dtr=dtr, pet=pet)
    print('hargreaves.npz', pet.shape, 'NaN PET', int(np.isnan(pet).sum()), 'zero PET', int((pet == 0).sum()))


def _gwam_loop(pet, precip, sm, sm0, spinup, monthly):
    """configurations.py:104-121 / components.py:298-357 for GWAM: the spin-up pass, then the simulation pass."""
    nc, nm = pet.shape
    s = types.SimpleNamespace(ncell=nc)
    out = {k: np.zeros((nc, nm)) for k in ('aet', 'q', 'sav')}
    prev = sm0.copy()
    for steps in (spinup, nm):
        for m in range(steps):
            P = np.copy(precip[:, m] if monthly else precip[:, steps - 1])
            _, a, q, sv = ref_gwam.runoffgen(pet[:, m], P, s, sm, prev)
            out['aet'][:, m], out['q'][:, m], out['sav'][:, m] = a, q, sv
            prev = np.copy(sv)
    return out


def golden_gwam():
    rng = np.random.default_rng(36)
    nm, spinup = 36, 12
    sm = rng.uniform(20, 400, NC)
    sm[::29] = 999.0                      # water bodies
    sm[7::61] = 0.0                       # no soil
    sm[11::73] = np.nan                   # missing capacity
    sm[13::17] = rng.uniform(1, 5, len(sm[13::17]))          # tiny capacity: B >= Sm often
    pet = rng.uniform(0, 180, (NC, nm))
    pet[rng.random(pet.shape) < 0.01] = np.nan
    precip = rng.gamma(1.2, 50.0, (NC, nm))
    precip[rng.random(precip.shape) < 0.02] = np.nan
    precip[::29][:, -1] = np.nan          # lakes with NaN P in the columns the reference driver reads
    precip[::29][:, spinup - 1] = np.nan
    precip[1::5] *= 0.05                  # dry cells: the 0.1 floor and Sav <= 0
    pet[2::5] *= 3.0
    sm0 = 0.5 * sm
    ref = _gwam_loop(pet, precip, sm, sm0, spinup, monthly=False)
    mon = _gwam_loop(pet, precip, sm, sm0, spinup, monthly=True)
    np.savez_compressed(os.path.join(HERE, 'gwam.npz'), pet=pet, precip=precip, sm=sm, sm0=sm0, spinup=spinup,
                        **{k: v for k, v in ref.items()}, **{'monthly_' + k: v for k, v in mon.items()})
    q, s = ref['q'], ref['sav']
    print('gwam.npz', 'Sav == 0:', int((s == 0).sum()), 'Sav == Sm:', int((s == sm[:, None]).sum()), 'NaN Q:',
          int(np.isnan(q).sum()))


def _drt_maps(root, w):
    """Routing inputs as 280 x 720 DRT-style maps (north to south, 68 rows up from the bottom, -9999 = no data): the only
    form the reference's loader reads on the 360 x 720 grid (data_load.py:392-425)."""
    rt = os.path.join(root, 'input', 'routing', 'mrtm')
    r_map = 280 - 1 - (w.coords[:, 4].astype(int) - 1 - 68)
    c_map = w.coords[:, 3].astype(int) - 1
    inside = (r_map >= 0) & (r_map < 280)
    for name, vec in (('flow_dist', w.flow_dist), ('velocity', w.velocity), ('flow_dir', w.flow_dir)):
        m = np.full((280, 720), -9999.0)
        m[r_map[inside], c_map[inside]] = vec[inside]
        np.save(os.path.join(rt, name + '.npy'), m)


def _tree_case(tag, root, ini, w, args=None):
    _drt_maps(root, w)
    settings = ConfigReader(ini)
    settings.update(args or {})
    settings.OutputUnitStr = 'mmpermonth'        # (the reference's reader derives it; its writer reads it)
    os.makedirs(settings.OutputFolder, exist_ok=True)
    c = RefRunner(settings).run()
    res = {tag + '_' + k: np.asarray(getattr(c, k)) for k in ('PET', 'AET', 'Q', 'Sav', 'ChStorage', 'Avg_ChFlow')}
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:
        for d, _, files in os.walk(os.path.join(root, 'input')):
            for fn in files:
                full = os.path.join(d, fn)
                z.write(full, os.path.relpath(full, root))
        z.write(ini, os.path.basename(ini))
    res[tag + '_tree_zip'] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    res[tag + '_old_root'] = np.array(root)
    res[tag + '_ini_name'] = np.array(os.path.basename(ini))
    return res


def golden_hgm():
    w = synth.make_world(nrow=360, ncol=720, ncell=150, n_basins=4, seed=3)
    y0, y1 = 1971, 1972
    f = synth.hgm_forcing(w, synth.make_forcing(w, 24, nan_precip=False))
    f['temp'][3, 2], f['dtr'][4, 3], f['dtr'][5, 4] = np.nan, -2.0, np.nan
    out = {}
    with tempfile.TemporaryDirectory() as root:
        ini = synth.write_hgm_example(root, w, f, y0, y1, runoff_spinup=12, routing_spinup=6, output_vars=('q',))
        out.update(_tree_case('hist', root, ini, w))
    rng = np.random.default_rng(8)
    with tempfile.TemporaryDirectory() as root:
        ini = synth.write_hgm_example(root, w, f, y0, y1, runoff_spinup=6, routing_spinup=12, output_vars=('q',),
                                      hist_flag=False, sav=rng.uniform(0, 300, (w.ncell, 5)),
                                      ch_storage=rng.uniform(0, 1e6, (w.ncell, 3)))
        out.update(_tree_case('future', root, ini, w))
    with tempfile.TemporaryDirectory() as root:
        f3 = synth.hgm_forcing(w, synth.make_forcing(w, 36))          # (ABCD's spin-up needs >= 25 months, abcd.py:258-266)
        ini = synth.write_hgm_example(root, w, f3, y0, y1 + 1, runoff='abcd', runoff_spinup=30, routing_spinup=6,
                                      output_vars=('q',))
        out.update(_tree_case('abcd', root, ini, w))
    np.savez_compressed(os.path.join(HERE, 'hgm.npz'), **out)
    print('hgm.npz', {k: v.shape for k, v in out.items() if k.endswith('_Q')})


if __name__ == '__main__':
    import warnings
    warnings.simplefilter('ignore')
    golden_hargreaves()
    golden_gwam()
    golden_hgm()
