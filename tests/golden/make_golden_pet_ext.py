"""Generate the Hargreaves-Samani / Thornthwaite golden vectors in this directory from the REAL reference (JGCRI/xanthos
v2.4.1).

Run in the build container only (needs the reference checkout, which the GPU box does not have):

    python tests/golden/make_golden_pet_ext.py

The reference is imported unmodified, the way make_golden_hgm.py imports it (hargreaves_samani.py / thornthwaite.py by
file path, the package with a stub for ``configobj``).  Each fixture stores the crafted inputs AND the reference's
outputs; fixtures are data only.

  hs.npz            hargreaves_samani.execute on 512 cells from pole to pole x 36 months (1975-1977, 1976 a leap year)
                    with NaN, negative and +-inf tas / tmax / tmin and both arccos clamps (polar night and polar day)
  thornthwaite.npz  thornthwaite.execute over 1971-1976 and 1975-1977 on 512 cells with 0 degC rows, negative rows, NaN
                    and +-inf (after the loader's nan_to_num, data_load.py:137-138), the reference test's 40N vector, and
                    calc_daylight_hours of a common and of a leap year at every latitude
  pet_ext.npz       the reference's ConfigRunner on small hs_abcd_mrtm and thornthwaite_abcd_mrtm trees on the 360 x 720
                    geometry, settings from this package's ConfigReader; the trees as zips
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

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


ref_hs = _load('ref_hs', 'xanthos/pet/hargreaves_samani.py')
ref_trn = _load('ref_trn', 'xanthos/pet/thornthwaite.py')

import make_golden_hgm as hgm  # noqa: E402  (stubs configobj, imports the reference's ConfigRunner)
from xanthos_amd import synth  # noqa: E402

NC = 512


def _lats(rng):
    return np.concatenate([[90.0, -90.0, 0.0, 89.5, -89.5, 66.6, -66.6, 70.0, -70.0, 23.4, 80.0, -80.0],
                           rng.uniform(-90, 90, NC - 12)])


def golden_hs():
    rng = np.random.default_rng(1975)
    y0, y1, nm = 1975, 1977, 36
    lat = _lats(rng)
    tas = rng.uniform(-15, 40, (NC, nm))
    tmin = tas - rng.uniform(0, 15, (NC, nm))
    tmax = tas + rng.uniform(0, 15, (NC, nm))
    tmax[rng.random(tmax.shape) < 0.05] -= 40.0            # tmax < tmin: the reference takes |tmax - tmin|
    for a in (tas, tmax, tmin):
        a[rng.random(a.shape) < 0.02] = np.nan
    tas[3, 4], tas[4, 5], tas[13, 7], tmax[5, 6], tmax[6, 7], tmin[7, 8], tmin[8, 9] = (np.inf, -np.inf, -0.0, np.inf,
                                                                                        -np.inf, np.inf, -np.inf)
    tas[2, :12] = 0.0
    cfg = types.SimpleNamespace(ncell=NC, nmonths=nm, StartYear=y0, EndYear=y1)
    data = types.SimpleNamespace(coords=np.stack([np.arange(NC), np.zeros(NC), lat], axis=1), hs_tas=tas.copy(),
                                 hs_tmax=tmax.copy(), hs_tmin=tmin.copy())
    pet = ref_hs.execute(cfg, data)
    np.savez_compressed(os.path.join(HERE, 'hs.npz'), start_year=y0, end_year=y1, lat=lat, tas=tas, tmax=tmax, tmin=tmin,
                        pet=pet)
    print('hs.npz', pet.shape, 'NaN PET', int(np.isnan(pet).sum()), 'zero PET', int((pet == 0).sum()))


def golden_thornthwaite():
    rng = np.random.default_rng(1976)
    lat_deg = _lats(rng)
    lat = np.radians(lat_deg)
    out = {'lat': lat}
    for tag, y0, y1 in (('a', 1971, 1976), ('b', 1975, 1977)):
        nm = 12 * (y1 - y0 + 1)
        tas = rng.uniform(-10, 35, (NC, nm))
        tas[rng.random(tas.shape) < 0.02] = np.nan
        tas[0, :] = 0.0                                    # I == 0 everywhere
        tas[1, :] = -3.0                                   # negative rows
        tas[2, 12:24] = 0.0                                # one year at 0 degC
        tas[20, 5], tas[21, 6], tas[22, 7] = np.inf, -np.inf, np.nan
        loaded = np.nan_to_num(tas)                        # data_load.py:137-138
        out[tag + '_start_year'], out[tag + '_end_year'] = y0, y1
        out[tag + '_tas'] = tas
        out[tag + '_pet'] = ref_trn.execute(loaded.copy(), lat, y0, y1)
    out['dl_common'] = ref_trn.calc_daylight_hours([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], lat)
    out['dl_leap'] = ref_trn.calc_daylight_hours([31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], lat)
    np.savez_compressed(os.path.join(HERE, 'thornthwaite.npz'), **out)
    print('thornthwaite.npz', {k: v.shape for k, v in out.items() if k.endswith('_pet')},
          'NaN PET', int(np.isnan(out['a_pet']).sum() + np.isnan(out['b_pet']).sum()))


def golden_pet_ext():
    w = synth.make_world(nrow=360, ncol=720, ncell=150, n_basins=4, seed=3)
    y0, y1 = 1975, 1977
    f = synth.pet_ext_forcing(w, synth.make_forcing(w, 36, nan_precip=False))
    f['tas'][3, 2], f['tas'][4, 3] = -4.0, -1.5
    out = {}
    with tempfile.TemporaryDirectory() as root:
        ini = synth.write_pet_ext_example(root, w, f, y0, y1, pet='hs', runoff_spinup=30, routing_spinup=6,
                                          output_vars=('q',))
        out.update(hgm._tree_case('hs', root, ini, w))
    f['tas'][5, 4] = np.nan
    with tempfile.TemporaryDirectory() as root:
        ini = synth.write_pet_ext_example(root, w, f, y0, y1, pet='thornthwaite', runoff_spinup=30, routing_spinup=6,
                                          output_vars=('q',))
        out.update(hgm._tree_case('trn', root, ini, w))
    np.savez_compressed(os.path.join(HERE, 'pet_ext.npz'), **out)
    print('pet_ext.npz', {k: v.shape for k, v in out.items() if k.endswith('_Q')})


if __name__ == '__main__':
    import warnings
    warnings.simplefilter('ignore')
    golden_hs()
    golden_thornthwaite()
    golden_pet_ext()
