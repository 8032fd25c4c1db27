#!/usr/bin/env python
"""Generate pm_edges.npz from the REAL reference (JGCRI/xanthos v2.4.1): run_pmpet on the Penman-Monteith edge case set.

Run in the build container only (needs /root/reference, which does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pm_edges.py

penman_monteith.py is imported unmodified by file path, like make_golden.py does.  The inputs are tests/pm_cases.py's
(1,280 one-hot cells x 1994-1996, eight classes with one edge each); the generator rebuilds them bit for bit on any
machine, so the fixture holds their SHA-256 instead of the arrays, and PET for five (water_idx, snow_idx) pairs: the
default (0, 6), swapped (6, 0), (2, 7), and the ties (3, 3) and (6, 6).

With one class per cell, PET of another pair differs from PET of (0, 6) only in the (cell, year) blocks whose class is
named by either pair, so the file holds (0, 6) whole and of every other pair the blocks that differ in bits from (0, 6):
``blocks_W_S`` (indices into the [ncell * nyears, 12] view) and ``values_W_S``; tests/pm_cases.py::golden_pet puts them
together again.  Fixtures are data only.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import pm_cases  # noqa: E402


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref_pm = _load('ref_pm', 'xanthos/pet/penman_monteith.py')
    cs = pm_cases.case_set()
    out = {'digest': np.array(cs.digest), 'start_year': cs.start_year, 'end_year': cs.end_year, 'nlcs': cs.nlcs,
           'lc_years': np.array(cs.lc_years), 'pairs': np.array(pm_cases.INDEX_PAIRS)}
    base = None
    for wi, si in pm_cases.INDEX_PAIRS:
        d = types.SimpleNamespace(**vars(cs.data))          # the reference writes its yearly slices into the bag
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                 # 0 / 0 behind np.where, like every run of the reference
            pet = ref_pm.run_pmpet(d, cs.ncell, cs.nlcs, cs.start_year, cs.end_year, wi, si, cs.lc_years)
        assert pet.shape == (cs.ncell, cs.nmonths) and np.isfinite(pet).all()
        if base is None:
            base = pet
            out['pet_0_6'] = pet
            continue
        a, b = pet.reshape(-1, 12).view(np.uint64), base.reshape(-1, 12).view(np.uint64)
        blocks = np.nonzero((a != b).any(axis=1))[0]
        out['blocks_{}_{}'.format(wi, si)] = blocks.astype(np.int32)
        out['values_{}_{}'.format(wi, si)] = pet.reshape(-1, 12)[blocks]
        print((wi, si), len(blocks), 'of', a.shape[0], 'blocks differ from (0, 6)')
    path = os.path.join(HERE, 'pm_edges.npz')
    np.savez_compressed(path, **out)
    print('pm_edges.npz', base.shape, float(base.min()), float(base.max()), os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
