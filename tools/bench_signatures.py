"""The flow duration curve and the regime signatures in HBM (``xh_signatures``) against the path they replace, at full size
(67,420 cells x 600 months).

    python tools/bench_signatures.py [--cells 67420] [--months 600] [--reps 7] [--sample 2000] [--no-host]   # writes the JSON

On a seeded seasonal gamma field with 2 % zeros (ties), plus 5 % of the cells all zero (deserts) and 1 % of the months NaN in
a tenth of the cells, the nine default exceedance percents:
(a) the kernel with all outputs (the table, the duration curve, the calendar means) and with the table alone; the library's
    ``signatures`` timer, the median of ``--reps`` calls after one warm-up, and their spread;
(b) the floor: a device-to-device copy of the same input in the same run (host clock around a synchronised call, the same
    repetitions) -- the kernel reads the input once and writes 6 % of it, so half the copy's time is what one read costs;
(c) the path it replaces, on this host: the array downloaded (host clock), then the numpy restatement of the definition,
    tests/signatures_np.py, which walks the rows one by one: timed on ``--sample`` rows and scaled to all of them (said so in
    the JSON); the same rows of the device's outputs are compared with it bit for bit, the two bounded columns in the measures
    of tests/test_signatures_host.py.
It records, it does not gate.  Results: profiles/signatures/bench_signatures.json; the table stands in
profiles/signatures/README.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from xanthos_amd import _hip, signatures      # noqa: E402


def make_field(ncell, nmonths, seed=5):
    rng = np.random.default_rng(seed)
    shape = rng.uniform(0.6, 8.0, (ncell, 1)).astype(np.float32)
    season = 1.0 + 0.6 * np.sin(2 * np.pi * (np.arange(nmonths) % 12) / 12.0 + rng.uniform(0, 6.28, (ncell, 1)))
    x = rng.standard_gamma(shape, (ncell, nmonths)) * (30.0 / shape) * season
    x[rng.random((ncell, nmonths)) < 0.02] = 0.0
    x[rng.random(ncell) < 0.05] = 0.0
    gaps = rng.random(ncell) < 0.1
    x[gaps] = np.where(rng.random((int(gaps.sum()), nmonths)) < 0.01, np.nan, x[gaps])
    return np.ascontiguousarray(x, dtype=np.float64)


def timer_ms(ctx, call, reps):
    out = []
    for _ in range(reps + 1):
        ctx.timing_reset()
        call()
        ctx.sync()
        out.append(ctx.timing('signatures')[0])
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
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sample', type=int, default=2000)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'signatures', 'bench_signatures.json'))
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    x = make_field(a.cells, a.months)
    ny = a.months // 12
    probs = signatures.probabilities()
    P = 2
    while P < 12 * ny:
        P *= 2
    d_x, d_copy = ctx.upload(x), ctx.empty((a.cells, a.months))
    d_table, d_fdc, d_regime = ctx.empty((a.cells, 18)), ctx.empty((a.cells, probs.size)), ctx.empty((a.cells, 12))
    res = {'device': ctx.name(), 'cells': a.cells, 'months': a.months, 'years': ny, 'reps': a.reps,
           'exceedance': list(signatures.EXCEEDANCE), 'input_bytes': int(x.nbytes),
           'output_bytes': int(8 * a.cells * (18 + probs.size + 12)), 'lds_bytes_per_workgroup': (P + 768 + ny + 32) * 8, 'kernel': {}}

    def call(outputs):
        ctx.signatures(a.cells, a.months, 0, ny, 0, probs, d_x, d_table, d_fdc if outputs else None, d_regime if outputs else None)
    for outputs in (True, False):
        key = 'all outputs' if outputs else 'the table alone'
        res['kernel'][key] = stats(timer_ms(ctx, lambda: call(outputs), a.reps))
        print('{:20s} {:8.3f} ms (min {:.3f}, max {:.3f})'.format(key, *[res['kernel'][key][k] for k in ('median_ms', 'min_ms', 'max_ms')]))
    res['copy_of_the_input'] = stats(clock_ms(ctx, lambda: ctx.d2d(d_copy, d_x), a.reps))
    res['kernel_over_copy'] = res['kernel']['all outputs']['median_ms'] / res['copy_of_the_input']['median_ms']
    print('device copy of the input ({} MB): {:.3f} ms; the kernel (all outputs) takes {:.2f} x that'.format(
        x.nbytes // 1000000, res['copy_of_the_input']['median_ms'], res['kernel_over_copy']))
    call(True)
    ctx.sync()
    got = d_table.download(), d_fdc.download(), d_regime.download()
    # a second call gives the same bytes (the grid is capped: every workgroup walks several rows)
    call(True)
    ctx.sync()
    res['two_calls_identical'] = all(u.tobytes() == v.tobytes() for u, v in zip(got, (d_table.download(), d_fdc.download(), d_regime.download())))

    if not a.no_host:
        import signatures_np as snp
        t0 = time.perf_counter()
        host = d_x.download()
        res['download_ms'] = (time.perf_counter() - t0) * 1e3
        rows = np.sort(np.random.default_rng(1).choice(a.cells, size=min(a.sample, a.cells), replace=False))
        t0 = time.perf_counter()
        want = snp.signatures(host[rows], 0, ny, 0, probs)
        sample_s = time.perf_counter() - t0
        res['host_numpy_sample_s'] = sample_s
        res['host_numpy_s_scaled_from_the_sample'] = sample_s * a.cells / rows.size
        bit = [c for c in range(18) if c not in (8, 13)]
        with np.errstate(invalid='ignore'):
            slope = np.abs(got[0][rows, 8] - want[0][:, 8]) / np.maximum(np.abs(want[0][:, 8]), 1.0)
            d = np.abs(got[0][rows, 13] - want[0][:, 13])
            centroid = np.minimum(d, 12.0 - d) * want[0][:, 14]
        res['sample'] = {'rows': int(rows.size), 'masks_identical': bool(np.array_equal(np.isnan(got[0][rows]), np.isnan(want[0]))),
                         'sixteen_columns_bit_for_bit': same_bits(got[0][rows][:, bit], want[0][:, bit]),
                         'fdc_bit_for_bit': same_bits(got[1][rows], want[1]), 'regime_bit_for_bit': same_bits(got[2][rows], want[2]),
                         'fdc_slope_max_distance_from_numpy': float(np.nanmax(slope)),
                         'centroid_max_distance_from_numpy': float(np.nanmax(centroid))}
        res['speedup'] = (res['host_numpy_s_scaled_from_the_sample'] + res['download_ms'] * 1e-3) / (res['kernel']['all outputs']['median_ms'] * 1e-3)
        print('host: download {:.1f} ms + numpy {:.2f} s on {} rows ({:.1f} s scaled to all); sample: {}'.format(
            res['download_ms'], sample_s, rows.size, res['host_numpy_s_scaled_from_the_sample'], res['sample']))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
