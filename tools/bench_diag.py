"""Per-kernel times of the diagnostics and time-series post-processors at the 0.5-degree grid size: 67,420 cells x 720
months in HBM (ctx.timing: HIP events around each launch, median of --reps), the host-side wall time of Diagnostics and of
TimeSeriesPlot around them (rendering stubbed out, then one PNG rendered on its own), and the wall time of run_model() on a
smaller synthetic tree with both switches off and on.

    python tools/bench_diag.py [--reps 10] [--model-ncell 5000]
"""
import argparse
import json
import logging
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))


def _model_time(root, ncell, on):
    from xanthos_amd import synth
    from xanthos_amd.model import Xanthos
    w = synth.make_world(nrow=360, ncol=720, ncell=ncell, n_basins=20, seed=9)
    f = synth.make_forcing(w, 120, nan_precip=False)
    ini = synth.write_example(root, w, f, 1971, 1980, runoff_spinup=36, routing_spinup=12, aggregates=True)
    if on:
        synth.write_diag_inputs(root, w, seed=3)
        synth.enable_diagnostics(ini, diag_scale=0, plot_scale=0, map_id=[0])      # 3 scales x 2 PNGs
    logging.disable(logging.INFO)
    Xanthos(ini).execute()                                  # warm: plans, code objects
    t = time.time()
    c = Xanthos(ini).execute()
    wall = time.time() - t
    logging.disable(logging.NOTSET)
    return wall, c.timings.get('post', 0.0), c.timings.get('plots', 0.0)


def main():
    from xanthos_amd import _hip
    from xanthos_amd.diagnostics import diagnostics, time_series
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--ncell', type=int, default=67420)
    ap.add_argument('--nmonths', type=int, default=720)
    ap.add_argument('--model-ncell', type=int, default=5000)
    a = ap.parse_args()
    ncell, nm = a.ncell, a.nmonths
    ctx = _hip.get_context(0)
    rng = np.random.default_rng(1)
    q = rng.lognormal(1.0, 1.2, (ncell, nm))
    q[rng.choice(ncell, ncell // 1000, replace=False), 7] = np.nan
    ref = SimpleNamespace(area=rng.uniform(100.0, 3000.0, ncell), vic=rng.lognormal(-3.0, 1.0, (ncell, 30)),
                          unh=rng.lognormal(-3.0, 1.0, ncell),
                          wbmd=np.stack([np.arange(1, ncell + 1), rng.lognormal(-3.0, 1.0, ncell)], axis=1),
                          wbmc=np.stack([np.arange(1, ncell + 1), rng.lognormal(-3.0, 1.0, ncell)], axis=1),
                          basin_ids=rng.integers(0, 236, ncell), country_ids=rng.integers(0, 250, ncell),
                          region_ids=rng.integers(0, 33, ncell),
                          basin_names=np.array(['Basin {}'.format(k) for k in range(1, 236)]),
                          country_names=np.array(['Country {}'.format(k) for k in range(249)]),
                          region_names=np.array(['Region {}'.format(k) for k in range(1, 33)]))
    d_q, d_ac = ctx.upload(q), ctx.upload(q * 3.0)
    d_out = ctx.empty((ncell,))
    samples = {k: [] for k in ('diag_cell_total_Q', 'diag_group_sum', 'agg_spatial')}
    walls = {'diagnostics': [], 'time_series_tables': []}
    stub = lambda *args: None                               # noqa: E731
    render, time_series.Plot_TS = time_series.Plot_TS, stub
    with tempfile.TemporaryDirectory() as root:
        s = SimpleNamespace(PerformDiagnostics=1, CreateTimeSeriesPlot=1, OutputFolder=root, StartYear=1951, EndYear=2010,
                            DiagnosticScale=0, TimeSeriesScale=0, TimeSeriesMapID=999, OutputInYear=0, OutputUnit=0,
                            device=0)
        for r in range(a.reps + 1):
            ctx.timing_reset()
            ctx.diag_cell_total(ncell, nm, d_q, 60.0, None, 1e6, d_out)           # the Q reduction alone
            if r >= 1:
                samples['diag_cell_total_Q'].append(ctx.timing('diag_cell_total')[0])
            ctx.timing_reset()
            t = time.time()
            diagnostics.Diagnostics(s, d_q, ref)
            t1 = time.time()
            time_series.TimeSeriesPlot(s, d_q, d_ac, ref)
            t2 = time.time()
            if r >= 1:
                walls['diagnostics'].append(t1 - t)
                walls['time_series_tables'].append(t2 - t1)
                samples['diag_group_sum'].append(ctx.timing('diag_group_sum')[0])     # 3 scales
                samples['agg_spatial'].append(ctx.timing('agg_spatial')[0])           # q + ac x 3 scales
        time_series.Plot_TS = render
        _, x = time_series.time_axis(s)
        t = time.time()
        time_series.Plot_TS(q[0], os.path.join(root, 'one'), 'runoff', 'month', 'mm', x)
        png_s = time.time() - t
    for b in (d_q, d_ac, d_out):
        b.free()
    res = {'ncell': ncell, 'nmonths': nm, 'device': ctx.name()}
    q_bytes = ncell * nm * 8
    for k, v in samples.items():
        res[k + '_ms'] = round(float(np.median(v)), 4)
        extra = ''
        if k == 'diag_cell_total_Q':
            gbs = q_bytes / (res[k + '_ms'] * 1e-3) / 1e9
            res['diag_cell_total_Q_GBs'] = round(gbs, 1)
            extra = '  {:.0f} GB/s, {:.0%} of 6.3 TB/s'.format(gbs, gbs / 6300.0)
        print('{:18s} {:8.4f} ms{}'.format(k, res[k + '_ms'], extra))
    for k, v in walls.items():
        res[k + '_wall_s'] = round(float(np.median(v)), 3)
        print('{} wall {:.3f} s'.format(k, res[k + '_wall_s']))
    res['png_720_months_s'] = round(png_s, 3)
    print('one 720-month PNG at 300 dpi: {:.3f} s'.format(png_s))
    for on in (False, True):
        with tempfile.TemporaryDirectory() as root:
            wall, post, plots = _model_time(root, a.model_ncell, on)
        key = 'run_model_diag_{}'.format('on' if on else 'off')
        res[key + '_s'], res[key + '_post_s'], res[key + '_plots_s'] = round(wall, 3), round(post, 3), round(plots, 3)
        print('run_model ({} cells x 120 months, diagnostics + plots {}): {:.3f} s, post {:.3f} s, plots {:.3f} s'.format(
            a.model_ncell, 'on' if on else 'off', wall, post, plots))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
