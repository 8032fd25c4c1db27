#!/usr/bin/env python
"""Generate gwam_edges.npz from the REAL reference (JGCRI/xanthos v2.4.1): runoffgen on the GWAM edge case sets.

Run in the build container only (needs /root/reference, which does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gwam_edges.py

gwam.py is imported unmodified by file path, like make_golden_hgm.py does.  The inputs are tests/gwam_cases.py's:

  a_*      set A (one month, one case per cell, water-body code 999): ch, p, pet, sm -> aet, q, sav
  alt_*    the hand-written rows under another water-body code (``alt_indexing``)
  b_*      a slice of set B (``b_cells``, every 13th cell: all classes, all initial storages) marched by the reference
           driver's month loop (spin-up pass, then simulation) with ``b_spinup`` months of spin-up, one precipitation column
           per pass (``b_ref_*``) and month m's column in month m (``b_mon_*``)

Fixtures are data only.
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
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import gwam_cases  # noqa: E402


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_gwam = _load('ref_gwam', 'xanthos/runoff/gwam.py')


def _month(cs):
    s = types.SimpleNamespace(ncell=cs.ncell)
    _, a, q, sv = ref_gwam.runoffgen(np.copy(cs.pet), np.copy(cs.p), s, np.copy(cs.sm), np.copy(cs.ch), cs.indexing)
    return {'ch': cs.ch, 'p': cs.p, 'pet': cs.pet, 'sm': cs.sm, 'aet': a, 'q': q, 'sav': sv}


def _loop(pet, precip, sm, sm0, spinup, monthly):
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


def main():
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # NaN comparisons, like every run of the reference
        a, alt = gwam_cases.set_a(), gwam_cases.set_a_alt()
        out.update({'a_' + k: v for k, v in _month(a).items()})
        out.update({'alt_' + k: v for k, v in _month(alt).items()})
        out['alt_indexing'] = alt.indexing
        b = gwam_cases.set_b()
        idx = gwam_cases.GOLDEN_B_CELLS
        pet, precip, sm, sm0 = b.pet[idx], b.precip[idx], b.sm[idx], b.sm0[idx]
        out.update(b_cells=idx.astype(np.int32), b_pet=pet, b_precip=precip, b_sm=sm, b_sm0=sm0,
                   b_spinup=gwam_cases.GOLDEN_B_SPINUP)
        for tag, monthly in (('ref', False), ('mon', True)):
            r = _loop(pet, precip, sm, sm0, gwam_cases.GOLDEN_B_SPINUP, monthly)
            out.update({'b_{}_{}'.format(tag, k): v for k, v in r.items()})
    path = os.path.join(HERE, 'gwam_edges.npz')
    np.savez_compressed(path, **out)
    print('gwam_edges.npz', 'A', a.ncell, 'alt', alt.ncell, 'B', pet.shape, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
