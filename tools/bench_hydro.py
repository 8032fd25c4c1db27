"""Per-kernel times of the hydropower post-processors at the 0.5-degree grid size: 67,420 cells x 600 months of routed flow
in HBM and 1,593 synthetic dams (ctx.timing: HIP events around each launch, median of --reps), the host-side wall time of
HydropowerPotential / HydropowerActual around them, and the wall time of run_model() on a smaller synthetic tree with both
switches off and on.

    python tools/bench_hydro.py [--reps 10] [--model-ncell 5000]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))


def _world(ncell, seed):
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(360 * 720, ncell, replace=False))
    rows, cols = flat % 360, flat // 360
    coords = np.stack([np.arange(1, ncell + 1), -180 + (cols + 0.5) * 0.5, -90 + (rows + 0.5) * 0.5], axis=1)
    return SimpleNamespace(ncell=ncell, coords=coords)


def _model_time(root, ncell, hydro):
    import logging
    from xanthos_amd import synth
    from xanthos_amd.model import Xanthos
    w = synth.make_world(nrow=360, ncol=720, ncell=ncell, n_basins=20, seed=9)
    f = synth.make_forcing(w, 120, nan_precip=False)
    ini = synth.write_example(root, w, f, 1971, 1980, runoff_spinup=36, routing_spinup=12, output_vars=('q',))
    if hydro:
        synth.write_hydro_inputs(root, w, ndams=200, seed=3)
        synth.enable_hydro(ini)
    logging.disable(logging.INFO)
    Xanthos(ini).execute()                                  # warm: plans, code objects
    t = time.time()
    c = Xanthos(ini).execute()
    wall = time.time() - t
    logging.disable(logging.NOTSET)
    return wall, c.timings.get('post', 0.0)


def main():
    from xanthos_amd import _hip, synth
    from xanthos_amd.hydropower import actual, potential
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--ncell', type=int, default=67420)
    ap.add_argument('--nmonths', type=int, default=600)
    ap.add_argument('--ndams', type=int, default=1593)
    ap.add_argument('--model-ncell', type=int, default=5000)
    a = ap.parse_args()
    ncell, nm = a.ncell, a.nmonths
    ctx = _hip.get_context(0)
    rng = np.random.default_rng(1)
    names = ('hpot_qmax', 'hpot_energy', 'hpot_region', 'hact_inflow', 'hact_sim')
    samples = {k: [] for k in names}
    walls = {'potential': [], 'actual': []}
    with tempfile.TemporaryDirectory() as root:
        hyd = synth.write_hydro_inputs(root, _world(ncell, 2), ndams=a.ndams, seed=5)
        s = SimpleNamespace(GridData=os.path.join(hyd, 'gridData.csv'), q_ex=0.9, ef=0.85, hpot_start_date='1/1951',
                            HydroDamData=os.path.join(hyd, 'resData_1593.csv'),
                            DrainArea=os.path.join(hyd, 'DRT_half_SourceArea_globe_float.txt'),
                            MissingCap=os.path.join(hyd, 'simulated_cap_by_country.csv'),
                            rule_curves=os.path.join(hyd, 'rule_curves_1593.npy'), hact_start_date='1/1951',
                            OutputFolder=os.path.join(root, 'out'), ProjectName='bench', device=0)
        import pandas as pd
        dams = actual.find_grid_ids(pd.read_csv(s.GridData)[['ID', 'long', 'lati']], pd.read_csv(s.HydroDamData)) - 1
        q = rng.lognormal(4.0, 1.2, (ncell, nm))
        q[np.setdiff1d(rng.choice(ncell, ncell // 1000, replace=False), dams), 7] = np.nan    # NaN cells, none under a dam
        d_q = ctx.upload(q)
        for r in range(a.reps + 1):
            ctx.timing_reset()
            t = time.time()
            potential.HydropowerPotential(s, d_q)
            t1 = time.time()
            actual.HydropowerActual(s, d_q)
            t2 = time.time()
            if r >= 1:
                walls['potential'].append(t1 - t)
                walls['actual'].append(t2 - t1)
                for k in names:
                    ms, n = ctx.timing(k)
                    samples[k].append(ms)                   # all launches of the call (the region kernel runs twice)
    d_q.free()
    res = {'ncell': ncell, 'nmonths': nm, 'ndams': a.ndams, 'device': ctx.name()}
    for k, v in samples.items():
        res[k + '_ms'] = round(float(np.median(v)), 4)
        print('{:12s} {:8.4f} ms'.format(k, res[k + '_ms']))
    for k, v in walls.items():
        res[k + '_wall_s'] = round(float(np.median(v)), 3)
        print('HydropowerPotential' if k == 'potential' else 'HydropowerActual', 'wall {:.3f} s'.format(res[k + '_wall_s']))
    for hydro in (False, True):
        with tempfile.TemporaryDirectory() as root:
            wall, post = _model_time(root, a.model_ncell, hydro)
        key = 'run_model_hydro_{}'.format('on' if hydro else 'off')
        res[key + '_s'], res[key + '_post_s'] = round(wall, 3), round(post, 3)
        print('run_model ({} cells x 120 months, hydropower {}): {:.3f} s, post-processors {:.3f} s'.format(
            a.model_ncell, 'on' if hydro else 'off', wall, post))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
