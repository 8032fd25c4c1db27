"""The bootstrap intervals in HBM (``xh_extremes_boot``) against the two paths they replace, at full size (67,420 cells x 600
months, ``max``), and how often the intervals hold the truth.

    python tools/bench_extremes_boot.py [--cells 67420] [--months 600] [--reps 7] [--host-rows 64] [--coverage 4000] [--out FILE]

On the field of tools/bench_extremes.py (a seeded seasonal gamma field with 2 % zeros, 5 % of the cells all zero):
(a) the kernel: the library's ``extremes_boot`` timer, the median of ``--reps`` calls after one warm-up, for B in 100, 1000,
    2048 x nT in 0, 6, and the replicate fits per second (B x the rows that have a fit / the time);
(b) the obvious device route in the same session: B x the time of ``xh_extremes`` on the same input (its ``extremes`` timer,
    the same repetitions; without the B resampled arrays such a route would also have to make), and the ratio;
(c) the host route: the array downloaded (host clock), then the numpy restatement tests/exboot_np.py timed on ``--host-rows``
    rows with a fit and SCALED to the grid by rows -- a scaled figure, not a measurement of the whole grid;
(d) coverage: ``--coverage`` rows per case of GEV samples of known k (xi = 40, alpha = 12) at 30 and 50 years, B = 1000: the share of
    rows whose 90 % interval holds the true 20- and 100-year level.
It records, it does not gate.  Results: profiles/extremes_boot/bench_extremes_boot.json; the table stands in DESIGN 4.22."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_extremes import make_field, stats     # noqa: E402
from xanthos_amd import _hip, extremes           # noqa: E402


def timer_ms(ctx, name, call, reps):
    out = []
    for _ in range(reps + 1):
        ctx.timing_reset()
        call()
        ctx.sync()
        out.append(ctx.timing(name)[0])
    return out[1:]


def coverage(ctx, rows_per_case, B, seed=11):
    """{case: share of rows whose 90 % interval holds the true level} for GEV samples of known k."""
    xi, alpha, periods = 40.0, 12.0, (20.0, 100.0)
    out = {}
    for ny in (30, 50):
        for k in (-0.2, 0.0, 0.2):
            rng = np.random.default_rng(seed + ny + int(100 * k))
            u = -np.log(rng.random((rows_per_case, ny)))
            z = xi - alpha * np.log(u) if k == 0.0 else xi + alpha * (1.0 - u ** k) / k
            ci = extremes.bootstrap_rows(ctx, np.repeat(z, 12, axis=1), 'max', 0, ny, periods, 10, B, 0.90, seed)
            got = ci.download()
            ci.free()
            have = ~np.isnan(got[:, 1])
            case = {'rows_with_an_interval': float(have.mean())}
            for j, T in enumerate(periods):
                y = -np.log1p(-1.0 / T)
                true = xi - alpha * np.log(y) if k == 0.0 else xi + alpha * (1.0 - y ** k) / k
                case['x_T{:g}'.format(T)] = float(((got[have, 3 + 2 * j] <= true) & (true <= got[have, 4 + 2 * j])).mean())
            case['k'] = float(((got[have, 1] <= k) & (k <= got[have, 2])).mean())
            out['{} years, k = {:g}'.format(ny, k)] = case
            print('coverage, {} years, k = {:g}: {}'.format(ny, k, case), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=67420)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-rows', type=int, default=64)
    ap.add_argument('--coverage', type=int, default=4000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'extremes_boot', 'bench_extremes_boot.json'))
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    x = make_field(a.cells, a.months)
    ny = a.months // 12
    T = extremes.RETURN_PERIODS
    d_x = ctx.upload(x)
    d_table, d_annual, d_ty = ctx.empty((a.cells, 8 + len(T))), ctx.empty((a.cells, ny)), ctx.empty((a.cells, ny))
    res = {'device': ctx.name(), 'cells': a.cells, 'months': a.months, 'years': ny, 'reps': a.reps, 'kernel': {}}
    res['xh_extremes'] = stats(timer_ms(ctx, 'extremes', lambda: ctx.extremes(a.cells, a.months, 0, ny, 'max', 10, T, d_x, d_table, d_annual,
                                                                              d_ty), a.reps))
    fitted = ~np.isnan(d_table.download()[:, 5])
    res['rows_with_a_fit'] = int(fitted.sum())
    print('xh_extremes: {:.3f} ms; {} of {} rows have a fit'.format(res['xh_extremes']['median_ms'], res['rows_with_a_fit'], a.cells), flush=True)
    for B in (100, 1000, 2048):
        for nT in (0, len(T)):
            d_ci = ctx.empty((a.cells, 3 + 2 * nT))
            s = stats(timer_ms(ctx, 'extremes_boot', lambda: ctx.extremes_boot(a.cells, a.months, 0, ny, 'max', 10, T[:nT], B, 0.90, 1, d_x, d_ci),
                               a.reps))
            s['replicate_fits_per_s'] = B * res['rows_with_a_fit'] / (s['median_ms'] * 1e-3)
            s['B_calls_of_xh_extremes_ms'] = B * res['xh_extremes']['median_ms']
            s['ratio_to_B_calls_of_xh_extremes'] = s['B_calls_of_xh_extremes_ms'] / s['median_ms']
            res['kernel']['B = {}, nT = {}'.format(B, nT)] = s
            print('B = {:4d}, nT = {}: {:9.3f} ms (min {:.3f}, max {:.3f}), {:.3e} fits/s, {:.1f} x under B calls of xh_extremes'.format(
                B, nT, s['median_ms'], s['min_ms'], s['max_ms'], s['replicate_fits_per_s'], s['ratio_to_B_calls_of_xh_extremes']), flush=True)
            if B == 1000 and nT:
                ci = d_ci.download()
            d_ci.free()
    if a.host_rows:
        import exboot_np
        t0 = time.perf_counter()
        host = d_x.download()
        res['download_ms'] = (time.perf_counter() - t0) * 1e3
        rows = np.flatnonzero(fitted)[:a.host_rows]
        t0 = time.perf_counter()
        ref = exboot_np.bootstrap_rows(host[rows], 'max', T, 1000, 0.90, 1, min_years=10)[0]
        part = time.perf_counter() - t0
        res['host_numpy'] = {'rows': int(rows.size), 'B': 1000, 'seconds': part,
                             'SCALED_to_the_grid_s': part * res['rows_with_a_fit'] / rows.size}
        # (the rows of a slice draw as rows 0 .. of their own: compare nb and the masks only where the numbers agree)
        res['host_numpy']['ratio_to_the_kernel_scaled'] = (res['host_numpy']['SCALED_to_the_grid_s'] + res['download_ms'] * 1e-3) / (
            res['kernel']['B = 1000, nT = {}'.format(len(T))]['median_ms'] * 1e-3)
        first = rows[rows == np.arange(rows.size)]
        res['host_numpy']['rows_compared'] = int(first.size)
        if first.size:
            with np.errstate(invalid='ignore'):
                res['host_numpy']['nb_identical'] = bool(np.array_equal(ci[first, 0], ref[:first.size, 0]))
                res['host_numpy']['max_relative_difference_of_a_bound'] = float(np.nanmax(np.abs(ci[first, 1:] - ref[:first.size, 1:]) / np.abs(
                    ref[:first.size, 1:])))
        print('host: download {:.1f} ms; numpy on {} rows {:.2f} s, SCALED to the grid {:.0f} s'.format(
            res['download_ms'], rows.size, part, res['host_numpy']['SCALED_to_the_grid_s']), flush=True)
    if a.coverage:
        res['coverage_of_the_90_percent_interval'] = coverage(ctx, a.coverage, 1000)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
