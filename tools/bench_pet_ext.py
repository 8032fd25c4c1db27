"""Per-stage times of Hargreaves-Samani and Thornthwaite PET at the 0.5-degree grid size: 67,420 cells x 600 months,
synthetic forcing in HBM.  Prints ms and GB/s of algorithmic traffic per stage (ctx.timing: HIP events around each launch),
median of --reps.

    python tools/bench_pet_ext.py [--reps 20] [--daylight reference|monthly]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))


def main():
    from xanthos_amd import _hip
    from xanthos_amd.pet import hargreaves_samani, thornthwaite
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ncell', type=int, default=67420)
    ap.add_argument('--nmonths', type=int, default=600)
    ap.add_argument('--daylight', default='reference', choices=tuple(thornthwaite.DAYLIGHT_MODES))
    a = ap.parse_args()
    ncell, nm = a.ncell, a.nmonths
    y0, y1 = 1901, 1900 + nm // 12
    rng = np.random.default_rng(1)
    ctx = _hip.get_context(0)
    up = ctx.upload
    tas = rng.uniform(-20, 35, (ncell, nm))
    d_tas, d_tmax, d_tmin = up(tas), up(tas + rng.uniform(0, 8, (ncell, nm))), up(tas - rng.uniform(0, 8, (ncell, nm)))
    lat = rng.uniform(-60, 85, ncell)
    d_lat_deg, d_lat_rad = up(lat), up(np.radians(lat))
    nd = hargreaves_samani.days_per_month(y0, y1)
    d_pet = ctx.empty((ncell, nm))
    samples = {'hs_pet': [], 'trn_daylight': [], 'trn_pet': []}
    for r in range(a.reps + 2):
        ctx.timing_reset()
        hargreaves_samani.hs_device(ctx, ncell, nm, d_tas, d_tmax, d_tmin, d_lat_deg, nd, d_pet)
        thornthwaite.thornthwaite_device(ctx, ncell, nm, y0, d_tas, d_lat_rad, daylight=a.daylight, d_pet=d_pet)
        ctx.sync()
        if r >= 2:
            for k in samples:
                ms, n = ctx.timing(k)
                samples[k].append(ms / max(n, 1))
    cm = ncell * nm
    # algorithmic traffic: HS reads tas / tmax / tmin and writes PET; Thornthwaite reads tas and writes PET (the [ncell, 24]
    # daylight table it reads back is 13 MB); the daylight kernel writes its table
    nbytes = {'hs_pet': cm * 32, 'trn_daylight': ncell * 24 * 8, 'trn_pet': cm * 16}
    res = {'ncell': ncell, 'nmonths': nm, 'daylight': a.daylight, 'device': ctx.name()}
    for k, v in samples.items():
        ms = float(np.median(v))
        res[k] = {'ms': round(ms, 4), 'GBps': round(nbytes[k] / ms / 1e6, 1)}
        print('{:15s} {:8.4f} ms  {:7.1f} GB/s of {:.0f} MB'.format(k, ms, nbytes[k] / ms / 1e6, nbytes[k] / 1e6))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
