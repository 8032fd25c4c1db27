"""Per-stage times of Hargreaves PET and GWAM at the 0.5-degree grid size: 67,420 cells x 600 months, synthetic forcing in
HBM.  Prints ms and GB/s of algorithmic traffic per stage (ctx.timing: HIP events around each launch), median of --reps.

    python tools/bench_hgm.py [--reps 20] [--spinup 120] [--precipitation reference|monthly]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))


def main():
    from xanthos_amd import _hip
    from xanthos_amd.pet import hargreaves
    from xanthos_amd.runoff import gwam
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ncell', type=int, default=67420)
    ap.add_argument('--nmonths', type=int, default=600)
    ap.add_argument('--spinup', type=int, default=120)
    ap.add_argument('--precipitation', default='reference', choices=gwam.PRECIP_MODES)
    a = ap.parse_args()
    ncell, nm = a.ncell, a.nmonths
    rng = np.random.default_rng(1)
    ctx = _hip.get_context(0)
    up = ctx.upload
    d_t, d_d = up(rng.uniform(-20, 35, (ncell, nm))), up(rng.uniform(0, 15, (ncell, nm)))
    d_p, d_lat = up(rng.gamma(1.5, 40.0, (ncell, nm))), up(np.radians(rng.uniform(-60, 85, ncell)))
    sm = rng.uniform(10, 500, ncell)
    sm[::50] = 999.0
    d_sm, d_sm0 = up(sm), up(0.5 * sm)
    dec, dr, nd = hargreaves.month_factors(1901, 1900 + nm // 12)
    d_pet = ctx.empty((ncell, nm))
    out = {k: ctx.empty((ncell, nm)) for k in ('aet', 'q', 'sav')}
    samples = {'hargreaves_pet': [], 'gwam_spinup': [], 'gwam_sim': []}
    for r in range(a.reps + 2):
        ctx.timing_reset()
        hargreaves.hargreaves_device(ctx, ncell, nm, d_t, d_d, d_lat, dec, dr, nd, d_pet)
        gwam.gwam_device(ctx, ncell, nm, a.spinup, d_pet, d_p, d_sm, d_sm0, precipitation=a.precipitation, out=out)
        ctx.sync()
        if r >= 2:
            for k in samples:
                ms, n = ctx.timing(k)
                samples[k].append(ms / max(n, 1))
    cm = ncell * nm
    nbytes = {'hargreaves_pet': cm * 24, 'gwam_spinup': ncell * a.spinup * (16 if a.precipitation == 'monthly' else 8),
              'gwam_sim': cm * (40 if a.precipitation == 'monthly' else 32)}
    res = {'ncell': ncell, 'nmonths': nm, 'spinup': a.spinup, 'precipitation': a.precipitation, 'device': ctx.name()}
    for k, v in samples.items():
        ms = float(np.median(v))
        res[k] = {'ms': round(ms, 4), 'GBps': round(nbytes[k] / ms / 1e6, 1)}
        print('{:15s} {:8.4f} ms  {:7.1f} GB/s of {:.0f} MB'.format(k, ms, nbytes[k] / ms / 1e6, nbytes[k] / 1e6))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
