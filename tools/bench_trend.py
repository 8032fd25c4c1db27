"""The trend tables in HBM (``xh_trend``) against the path they replace, at full size (67,420 cells x 600 months).

    python tools/bench_trend.py [--cells 67420] [--months 600] [--reps 5] [--sample 64] [--no-host]   # writes the JSON

On a seeded seasonal gamma field with 2 % zeros (ties) and a weak trend, plus 5 % of the cells all zero (deserts):
(a) ``annual``: the years summed in HBM (``xh_agg_time``, np.sum's order) and the plain Mann-Kendall test on the 50 yearly
    values, 1,225 pairs per row; ``seasonal``: the seasonal Kendall test on the 600 months, 14,700 pairs per row.  The
    library's ``trend`` timer (and ``agg_time`` by the host clock around a synchronised call), the median of ``--reps`` calls.
(b) the path it replaces: the array downloaded (host clock), then per row ``scipy.stats.theilslopes`` -- per calendar month
    it gives no seasonal estimate, so for ``seasonal`` the baseline is the numpy statement of the definition,
    tests/trend_np.py, which forms and sorts all the slopes as theilslopes does -- and the numpy Mann-Kendall of
    tests/trend_np.py.  It is timed on a SAMPLE of ``--sample`` rows and SCALED to the grid: at full size it would take
    minutes to hours.  The sample's device rows are compared with it (nine columns equal, p relative).
It records, it does not gate.  Results: profiles/trend/bench_trend.json; the table stands in profiles/trend/README.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from xanthos_amd import _hip, trend      # noqa: E402


def make_field(ncell, nmonths, seed=5):
    rng = np.random.default_rng(seed)
    shape = rng.uniform(0.6, 8.0, (ncell, 1)).astype(np.float32)
    season = 1.0 + 0.6 * np.sin(2 * np.pi * (np.arange(nmonths) % 12) / 12.0 + rng.uniform(0, 6.28, (ncell, 1)))
    drift = 1.0 + rng.normal(0.0, 0.004, (ncell, 1)) * (np.arange(nmonths) / 12.0)
    x = rng.standard_gamma(shape, (ncell, nmonths)) * (30.0 / shape) * season * drift
    x[rng.random((ncell, nmonths)) < 0.02] = 0.0
    x[rng.random(ncell) < 0.05] = 0.0
    return np.ascontiguousarray(x, dtype=np.float64)


def median_ms(ctx, name, call, reps):
    out = []
    for _ in range(reps + 1):
        ctx.timing_reset()
        call()
        ctx.sync()
        out.append(ctx.timing(name)[0])
    return float(np.median(out[1:])), [float(v) for v in out[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=67420)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample', type=int, default=64)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'trend', 'bench_trend.json'))
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    x = make_field(a.cells, a.months)
    ny = a.months // 12
    z_conf = trend.z_of(0.95)
    d_x = ctx.upload(x)
    d_year = ctx.empty((a.cells, ny))
    d_out = ctx.empty((a.cells, 10))
    res = {'device': ctx.name(), 'cells': a.cells, 'months': a.months, 'reps': a.reps, 'series': {}}

    t = []
    for _ in range(a.reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.agg_time(a.cells, a.months, 12, 2, None, d_x, d_year)
        ctx.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    res['agg_time_ms_host_clock'] = float(np.median(t[1:]))
    runs = {'annual': lambda: ctx.trend(a.cells, ny, 0, ny, 1, z_conf, d_year, d_out),
            'seasonal': lambda: ctx.trend(a.cells, a.months, 0, a.months, 12, z_conf, d_x, d_out)}
    tables = {}
    for series, call in runs.items():
        ms, all_ms = median_ms(ctx, 'trend', call, a.reps)
        tables[series] = d_out.download()
        pairs = (ny * (ny - 1) // 2) * (1 if series == 'annual' else 12)
        ncol = ny if series == 'annual' else a.months
        res['series'][series] = {'trend_ms': ms, 'trend_ms_all': all_ms, 'pairs_per_row': pairs,
                                 'lds_bytes_per_workgroup': (ncol + 256 + 44) * 8 + 4096,
                                 'significant_at_5_percent': float(np.nanmean(tables[series][:, 4] < 0.05))}
        print('{:9s} {:9.3f} ms on the device ({} pairs per row)'.format(series, ms, pairs))

    if not a.no_host:
        import trend_np
        from scipy import stats
        t0 = time.perf_counter()
        host = d_x.download()
        res['download_ms'] = (time.perf_counter() - t0) * 1e3
        rows = np.random.default_rng(1).choice(a.cells, size=min(a.sample, a.cells), replace=False)
        yearly = host.reshape(a.cells, ny, 12).sum(axis=2)
        for series, arr, ns in (('annual', yearly, 1), ('seasonal', host, 12)):
            t0 = time.perf_counter()
            for r in rows:
                if ns == 1:
                    stats.theilslopes(arr[r], np.arange(ny), 0.95)
            t_theil = time.perf_counter() - t0
            t0 = time.perf_counter()
            ref = trend_np.trend_rows(arr[rows], ns, z_conf)
            t_np = time.perf_counter() - t0
            got = tables[series][rows]
            cols = [c for c in range(10) if c != 4]
            ok = bool(np.array_equal(got[:, cols], ref[:, cols], equal_nan=True))
            with np.errstate(invalid='ignore', divide='ignore'):
                perr = float(np.nanmax(np.where(ref[:, 4] > 0, np.abs(got[:, 4] - ref[:, 4]) / ref[:, 4], 0.0)))
            scaled = (t_theil + t_np) / len(rows) * a.cells
            s = res['series'][series]
            s.update(host_sample_rows=int(len(rows)), host_theilslopes_s_sample=t_theil, host_trend_np_s_sample=t_np,
                     host_s_scaled_to_grid=scaled, nine_columns_equal_on_sample=ok, p_max_rel_err_on_sample=perr,
                     speedup_scaled=(scaled + res['download_ms'] * 1e-3) / (s['trend_ms'] * 1e-3))
            print('{:9s} host: {:.1f} s scaled from {} rows; nine columns equal: {}; p rel err {:.2e}'.format(
                series, scaled, len(rows), ok, perr))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
