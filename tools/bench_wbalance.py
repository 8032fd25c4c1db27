"""The water balance and Budyko signatures in HBM (``xh_water_balance``) against the path they replace, at full size (67,420 cells
x 600 months, max_lag = 6).

    python tools/bench_wbalance.py [--cells 67420] [--months 600] [--reps 7] [--sample 2000] [--no-host]   # writes the JSON

On seeded fields -- a seasonal gamma precipitation with wet and dry years, a seasonal PET whose level differs from cell to cell
(aridity 0.2 .. 5), AET a fraction of the smaller of the two, runoff a noisy fraction of the rest -- with 1 % of the months NaN
in the runoff of a tenth of the cells:
(a) the kernel with all outputs (the table, the annual totals, the cross-correlation) and with the table alone; the library's
    ``water_balance`` timer, the median of ``--reps`` calls after one warm-up, and their spread;
(b) the yardstick: device-to-device copies of the same four inputs in the same run (host clock around a synchronised call, the
    same repetitions) -- the kernel reads the inputs once and writes 4 % of them, so half the copy's time is what one read costs;
(c) the path it replaces, on this host: the four arrays downloaded (host clock), then the numpy restatement of the definition,
    tests/wbalance_np.py, which walks the rows one by one: timed on ``--sample`` rows and scaled to all of them (said so in the
    JSON); the same rows of the device's outputs are compared with it bit for bit, the two bounded columns in the measures of
    tests/test_wbalance_host.py.
It records, it does not gate.  Results: profiles/water_balance/bench_wbalance.json; the table stands in
profiles/water_balance/README.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from xanthos_amd import _hip, waterbalance      # noqa: E402


def make_fields(ncell, nmonths, seed=6):
    rng = np.random.default_rng(seed)
    ny = nmonths // 12
    phase = rng.uniform(0, 6.28, (ncell, 1))
    season = (1.0 + 0.6 * np.sin(2 * np.pi * (np.arange(nmonths) % 12) / 12.0 + phase)).astype(np.float32)
    wet = np.repeat(rng.gamma(8.0, 1.0 / 8.0, (ncell, ny)).astype(np.float32), 12, axis=1)[:, :nmonths]
    p = rng.standard_gamma(4.0, (ncell, nmonths), dtype=np.float32) * 20.0 * wet * season
    level = np.exp(rng.uniform(np.log(0.2), np.log(5.0), (ncell, 1))).astype(np.float32)
    pet = 80.0 * level * (2.0 - season) * rng.uniform(0.9, 1.1, (ncell, nmonths)).astype(np.float32)
    aet = np.minimum(p, pet) * rng.uniform(0.7, 0.95, (ncell, nmonths)).astype(np.float32)
    q = (p - aet) * rng.uniform(0.8, 1.1, (ncell, nmonths)).astype(np.float32)
    gaps = rng.random(ncell) < 0.1
    q[gaps] = np.where(rng.random((int(gaps.sum()), nmonths)) < 0.01, np.nan, q[gaps])
    return [np.ascontiguousarray(v, dtype=np.float64) for v in (p, pet, q, aet)]


def timer_ms(ctx, call, reps):
    out = []
    for _ in range(reps + 1):
        ctx.timing_reset()
        call()
        ctx.sync()
        out.append(ctx.timing('water_balance')[0])
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


def same_bits(a, b):
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=67420)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--max-lag', type=int, default=6)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sample', type=int, default=2000)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'water_balance', 'bench_wbalance.json'))
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    fields = make_fields(a.cells, a.months)
    ny = a.months // 12
    P2 = 4
    while P2 < ny:
        P2 *= 2
    d_in = [ctx.upload(x) for x in fields]
    d_copy = [ctx.empty((a.cells, a.months)) for _ in fields]
    d_table, d_annual, d_xcorr = ctx.empty((a.cells, 21)), ctx.empty((a.cells, 4, ny)), ctx.empty((a.cells, a.max_lag + 1))
    res = {'device': ctx.name(), 'cells': a.cells, 'months': a.months, 'years': ny, 'max_lag': a.max_lag, 'reps': a.reps,
           'input_bytes': int(sum(x.nbytes for x in fields)), 'output_bytes': int(8 * a.cells * (21 + 4 * ny + a.max_lag + 1)),
           'lds_bytes_per_workgroup': (28 * ny + 2 * P2 + 1296) * 8, 'kernel': {}}

    def call(outputs):
        ctx.water_balance(a.cells, a.months, 0, ny, a.max_lag, waterbalance.OMEGA0, d_in[0], d_in[1], d_in[2], d_in[3], d_table,
                          d_annual if outputs else None, d_xcorr if outputs else None)
    for outputs in (True, False):
        key = 'all outputs' if outputs else 'the table alone'
        res['kernel'][key] = stats(timer_ms(ctx, lambda: call(outputs), a.reps))
        print('{:20s} {:8.3f} ms (min {:.3f}, max {:.3f})'.format(key, *[res['kernel'][key][k] for k in ('median_ms', 'min_ms', 'max_ms')]))

    def copy():
        for dst, src in zip(d_copy, d_in):
            ctx.d2d(dst, src)
    res['copy_of_the_inputs'] = stats(clock_ms(ctx, copy, a.reps))
    res['kernel_over_copy'] = res['kernel']['all outputs']['median_ms'] / res['copy_of_the_inputs']['median_ms']
    print('device copy of the inputs ({} MB): {:.3f} ms; the kernel (all outputs) takes {:.2f} x that'.format(
        res['input_bytes'] // 1000000, res['copy_of_the_inputs']['median_ms'], res['kernel_over_copy']))
    call(True)
    ctx.sync()
    got = d_table.download(), d_annual.download(), d_xcorr.download()
    # a second call gives the same bytes (the grid is capped: every workgroup walks several rows)
    call(True)
    ctx.sync()
    res['two_calls_identical'] = all(u.tobytes() == v.tobytes() for u, v in zip(got, (d_table.download(), d_annual.download(), d_xcorr.download())))

    if not a.no_host:
        import wbalance_np as wnp
        t0 = time.perf_counter()
        host = [d.download() for d in d_in]
        res['download_ms'] = (time.perf_counter() - t0) * 1e3
        rows = np.sort(np.random.default_rng(1).choice(a.cells, size=min(a.sample, a.cells), replace=False))
        t0 = time.perf_counter()
        want = wnp.water_balance(host[0][rows], host[1][rows], host[2][rows], host[3][rows], 0, ny, a.max_lag, waterbalance.OMEGA0)
        sample_s = time.perf_counter() - t0
        res['host_numpy_sample_s'] = sample_s
        res['host_numpy_s_scaled_from_the_sample'] = sample_s * a.cells / rows.size
        bit = [c for c in range(21) if c not in (11, 12)]
        with np.errstate(invalid='ignore'):
            omega = np.abs(got[0][rows, 11] - want[0][:, 11]) / np.abs(want[0][:, 11])
            dev = np.abs(got[0][rows, 12] - want[0][:, 12]) / np.maximum(np.abs(want[0][:, 12]), 1.0)
        res['sample'] = {'rows': int(rows.size), 'masks_identical': bool(np.array_equal(np.isnan(got[0][rows]), np.isnan(want[0]))),
                         'nineteen_columns_bit_for_bit': same_bits(got[0][rows][:, bit], want[0][:, bit]),
                         'annual_bit_for_bit': same_bits(got[1][rows], want[1]), 'xcorr_bit_for_bit': same_bits(got[2][rows], want[2]),
                         'rows_with_omega': int((~np.isnan(want[0][:, 11])).sum()),
                         'omega_max_distance_from_numpy': float(np.nanmax(omega)),
                         'budyko_dev_max_distance_from_numpy': float(np.nanmax(dev))}
        res['speedup'] = (res['host_numpy_s_scaled_from_the_sample'] + res['download_ms'] * 1e-3) / (res['kernel']['all outputs']['median_ms'] * 1e-3)
        print('host: download {:.1f} ms + numpy {:.2f} s on {} rows ({:.1f} s scaled to all); sample: {}'.format(
            res['download_ms'], sample_s, rows.size, res['host_numpy_s_scaled_from_the_sample'], res['sample']))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
