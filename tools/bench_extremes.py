"""The annual extremes in HBM (``xh_extremes``) against the path they replace, at full size (67,420 cells x 600 months).

    python tools/bench_extremes.py [--cells 67420] [--months 600] [--reps 7] [--sample 2000] [--no-host]   # writes the JSON

On a seeded seasonal gamma field with 2 % zeros (ties), plus 5 % of the cells all zero (deserts: no fit), six return periods:
(a) the kernel: ``max`` alone and ``max`` + ``min`` (two calls), with and without the two [ncell, nyear] outputs (the annual
    series and every year's return period); the library's ``extremes`` timer, the median of ``--reps`` calls after one
    warm-up, and their spread;
(b) the floor: a device-to-device copy of the same input in the same run (host clock around a synchronised call, the same
    repetitions) -- the kernel reads the input once and writes almost nothing, so half the copy's time is what one read costs;
(c) the path it replaces, on this host: the array downloaded (host clock), then the numpy restatement of the definition,
    tests/extremes_np.py, vectorised over the cells (``max``, the same six periods), timed once at full size; ``--sample``
    rows of the device's table are compared with it in the measures of tests/extremes_cases.py.
It records, it does not gate.  Results: profiles/extremes/bench_extremes.json; the table stands in profiles/extremes/README.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from xanthos_amd import _hip, extremes      # noqa: E402


def make_field(ncell, nmonths, seed=5):
    rng = np.random.default_rng(seed)
    shape = rng.uniform(0.6, 8.0, (ncell, 1)).astype(np.float32)
    season = 1.0 + 0.6 * np.sin(2 * np.pi * (np.arange(nmonths) % 12) / 12.0 + rng.uniform(0, 6.28, (ncell, 1)))
    x = rng.standard_gamma(shape, (ncell, nmonths)) * (30.0 / shape) * season
    x[rng.random((ncell, nmonths)) < 0.02] = 0.0
    x[rng.random(ncell) < 0.05] = 0.0
    return np.ascontiguousarray(x, dtype=np.float64)


def timer_ms(ctx, call, reps):
    out = []
    for _ in range(reps + 1):
        ctx.timing_reset()
        call()
        ctx.sync()
        out.append(ctx.timing('extremes')[0])
    return out[1:]


def clock_ms(ctx, call, reps):
    out = []
    for _ in range(reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms)), 'all_ms': [float(v) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=67420)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sample', type=int, default=2000)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'extremes', 'bench_extremes.json'))
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    x = make_field(a.cells, a.months)
    ny = a.months // 12
    T = extremes.RETURN_PERIODS
    d_x, d_copy = ctx.upload(x), ctx.empty((a.cells, a.months))
    d_table = {k: ctx.empty((a.cells, 8 + len(T))) for k in extremes.KINDS}
    d_annual, d_ty = ctx.empty((a.cells, ny)), ctx.empty((a.cells, ny))
    res = {'device': ctx.name(), 'cells': a.cells, 'months': a.months, 'years': ny, 'reps': a.reps, 'return_periods': list(T),
           'input_bytes': int(x.nbytes), 'lds_bytes_per_workgroup': 4 * (776 + 2 * ny) * 8, 'kernel': {}}

    def call(kinds, outputs):
        for k in kinds:
            ctx.extremes(a.cells, a.months, 0, ny, k, 10, T, d_x, d_table[k], d_annual if outputs else None, d_ty if outputs else None)
    for name, kinds in (('max', ('max',)), ('max+min', ('max', 'min'))):
        for outputs in (True, False):
            key = '{}, {} the [ncell, nyear] outputs'.format(name, 'with' if outputs else 'without')
            res['kernel'][key] = stats(timer_ms(ctx, lambda: call(kinds, outputs), a.reps))
            print('{:45s} {:8.3f} ms (min {:.3f}, max {:.3f})'.format(key, *[res['kernel'][key][k] for k in ('median_ms', 'min_ms', 'max_ms')]))
    res['copy_of_the_input'] = stats(clock_ms(ctx, lambda: ctx.d2d(d_copy, d_x), a.reps))
    res['kernel_over_copy'] = res['kernel']['max, without the [ncell, nyear] outputs']['median_ms'] / res['copy_of_the_input']['median_ms']
    print('device copy of the input ({} MB): {:.3f} ms; the kernel (max, no outputs) takes {:.2f} x that'.format(
        x.nbytes // 1000000, res['copy_of_the_input']['median_ms'], res['kernel_over_copy']))
    call(('max',), True)
    ctx.sync()
    table, T_year = d_table['max'].download(), d_ty.download()
    res['rows_with_a_fit'] = float(np.mean(~np.isnan(table[:, 5])))

    if not a.no_host:
        import extremes_cases as cases
        import extremes_np
        t0 = time.perf_counter()
        host = d_x.download()
        res['download_ms'] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ref = extremes_np.extremes_rows(host, 'max', T, min_years=10)
        res['host_numpy_s'] = time.perf_counter() - t0
        rows = np.sort(np.random.default_rng(1).choice(a.cells, size=min(a.sample, a.cells), replace=False))
        got = (table[rows], d_annual.download()[rows], T_year[rows])
        want = tuple(v[rows] for v in ref)
        err = cases.errors(got[0], got[2], want[0], want[2])
        res['sample'] = {'rows': int(rows.size), 'masks_identical': bool(cases.same_masks(*got, *want)),
                         'n_annual_l1_l2_t3_t4_bit_for_bit': bool(cases.bits_equal(got[0], got[1], want[0], want[1])),
                         'max_error': {q: float(np.nanmax(err[q])) for q in cases.QUANTITIES}}
        res['speedup'] = (res['host_numpy_s'] + res['download_ms'] * 1e-3) / (res['kernel']['max, with the [ncell, nyear] outputs']['median_ms'] * 1e-3)
        print('host: download {:.1f} ms + numpy {:.2f} s; sample of {} rows: {}'.format(res['download_ms'], res['host_numpy_s'],
                                                                                     rows.size, res['sample']))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
