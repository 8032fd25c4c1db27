#!/usr/bin/env python
"""Generate pet_edges.npz from the REAL reference (JGCRI/xanthos v2.4.1): the three simple PET modules on the edge case sets.

Run in the build container only (needs /root/reference, which does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pet_edges.py

hargreaves.py, hargreaves_samani.py and thornthwaite.py are imported unmodified by file path, like make_golden_hgm.py does.
The inputs are tests/pet_cases.py's and are not stored (the host test rebuilds them); the fixture holds outputs only:

  hg_a, hg_b      hargreaves.calculate_pet month by month on set A and on every 4th latitude of set B, after the harness's
                  preparation (nan_to_num of T and D); calculate_pet zeroes negative D itself
  hs_a, hs_b      hargreaves_samani.pet per element x the days of the month
  dl_a, dl_b      thornthwaite.calc_daylight_hours, common and leap year side by side [ncell, 24]
  tr_a_<year>     thornthwaite.execute on set A as a one-year run from <year>
  tr_b_<nyears>   thornthwaite.execute on the first cells of set B, nyears from 1896

calculate_pet and execute write into their arguments: they get copies.  Fixtures are data only.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

import pet_cases as C  # noqa: E402
import pet_np as P  # noqa: E402


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_hg = _load('ref_hg', 'xanthos/pet/hargreaves.py')
ref_hs = _load('ref_hs', 'xanthos/pet/hargreaves_samani.py')
ref_trn = _load('ref_trn', 'xanthos/pet/thornthwaite.py')


def _hg(cs, rows=slice(None)):
    temp, dtr, lat = np.nan_to_num(cs.temp[rows]), np.nan_to_num(cs.dtr[rows]), cs.lat[rows]
    out = np.zeros(temp.shape)
    for m in range(temp.shape[1]):
        out[:, m] = ref_hg.calculate_pet(np.copy(temp[:, m]), np.copy(dtr[:, m]), np.copy(lat), cs.dec[m], cs.dr[m], cs.nd[m])
    return out


def _hs(cs, rows=slice(None)):
    tas, tmax, tmin, lat = cs.tas[rows], cs.tmax[rows], cs.tmin[rows], cs.lat[rows]
    out = np.zeros(tas.shape)
    for c in range(tas.shape[0]):
        for m in range(tas.shape[1]):
            out[c, m] = ref_hs.pet(lat[c], m, tas[c, m], tmax[c, m], tmin[c, m])
    return out * cs.nd


def _dl(lat):
    return np.concatenate([ref_trn.calc_daylight_hours(P.MONTHDAYS, np.copy(lat)),
                           ref_trn.calc_daylight_hours(P.LEAP_MONTHDAYS, np.copy(lat))], axis=1)


def main():
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # NaN and inf arithmetic, like every run of the reference
        with np.errstate(all='ignore'):
            out['hg_a'] = _hg(C.cases('hg', 'a'))
            out['hg_b'] = _hg(C.cases('hg', 'b'), C.GOLDEN_B_LATS)
            out['hs_a'] = _hs(C.cases('hs', 'a'))
            out['hs_b'] = _hs(C.cases('hs', 'b'), C.GOLDEN_B_LATS)
            out['dl_a'] = _dl(C.cases('dl', 'a').lat)
            out['dl_b'] = _dl(C.cases('dl', 'b').lat[C.GOLDEN_B_LATS])
            a = C.cases('tr', 'a')
            for y in C.YEARS_A:
                out['tr_a_{}'.format(y)] = ref_trn.execute(np.copy(a.tas), np.copy(a.lat), y, y)
            for ny in C.NYEARS_B:
                b = C.cases('tr', 'b', ny)
                out['tr_b_{}'.format(ny)] = ref_trn.execute(np.copy(b.tas[C.GOLDEN_B_CELLS]), np.copy(b.lat[C.GOLDEN_B_CELLS]),
                                                            C.Y0_B, C.Y0_B + ny - 1)
    path = os.path.join(HERE, 'pet_edges.npz')
    np.savez_compressed(path, **out)
    print('pet_edges.npz', {k: v.shape for k, v in out.items()}, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
