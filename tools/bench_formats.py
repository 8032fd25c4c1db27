"""The array output formats at the 0.5-degree grid size: one monthly variable, 67,420 cells x 600 months in HBM.

    python tools/bench_formats.py [--reps 5] [--out profiles/out_formats]

Times (wall clock around calls that return when the file is complete; the five writers take turns, the first round warms
code objects, slots and the page cache and is dropped; median and range of the rest), all in one process:
  (a) npy      OutWriter.write() with OutputFormat 4: save_npy's path (header here, xh_download_files behind it) -- the
               yardstick, unchanged by the other formats
  (b) nc       OutputFormat 0: header here, xh_pack_f32_be into a scratch array, xh_download_files of half the bytes
  (c) mat      OutputFormat 2: header here, xh_transpose into a scratch array, xh_download_files
  (d) nc_host  the host route to (b)'s file: download, astype('>f4') on one core, header + bytes in one write
  (e)          xh_pack_f32_be alone (the library's timer "pack_f32_be") against xh_memcpy_d2d of the same array, as GB/s of
               the 12 bytes per value the kernel moves (16 for the copy)
The files of (b) and (d) are compared byte for byte.  With --out the table goes to <out>/README.md, the numbers to
<out>/bench_formats.json.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))


def spread(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'n': len(xs)}


def main():
    from xanthos_amd import _hip
    from xanthos_amd.data_writer import formats
    from xanthos_amd.data_writer.out_writer import OutWriter
    ap = argparse.ArgumentParser()
    ap.add_argument('--ncell', type=int, default=67420)
    ap.add_argument('--nmonths', type=int, default=600)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    rng = np.random.default_rng(1)
    q = rng.gamma(0.7, 40.0, (a.ncell, a.nmonths))             # like monthly runoff in mm
    q[rng.random(q.shape) < 0.01] = np.nan
    d_q = ctx.upload(q)
    n = q.size
    folder = tempfile.mkdtemp(prefix='bench_formats_')
    years = a.nmonths // 12

    def writer(fmt):
        s = SimpleNamespace(output_vars=['q'], ProjectName='bench', OutputFolder=folder, OutputFormat=fmt, OutputUnit=0,
                            OutputInYear=0, StartYear=1971, EndYear=1970 + years, device=0)
        return OutWriter(s, np.ones(a.ncell), {'q': d_q})

    host_path = os.path.join(folder, 'host_route.nc')

    def host_route():
        data = d_q.download()
        with np.errstate(over='ignore'):
            body = data.astype('>f4')
        with open(host_path, 'wb') as fh:
            fh.write(formats.nc_header(a.ncell, a.nmonths, 0, 'mmpermonth', 'q'))
            fh.write(memoryview(body).cast('B'))

    runs = (('npy', lambda: writer(4).write()), ('nc', lambda: writer(0).write()), ('mat', lambda: writer(2).write()),
            ('nc_host', host_route))
    walls = {name: [] for name, _ in runs}
    for rep in range(a.reps + 1):
        for name, run in runs:
            ctx.sync()
            t = time.perf_counter()
            run()
            dt = time.perf_counter() - t
            if rep:
                walls[name].append(dt)
    res = {'device': ctx.name(), 'ncell': a.ncell, 'nmonths': a.nmonths, 'array_bytes': int(q.nbytes)}
    paths = {k: os.path.join(folder, 'q_mmpermonth_bench.' + k) for k in ('npy', 'nc', 'mat')}
    for k, p in paths.items():
        res[k + '_bytes'] = os.path.getsize(p)
    for key, name in (('a_npy_write_s', 'npy'), ('b_nc_write_s', 'nc'), ('c_mat_write_s', 'mat'), ('d_nc_host_route_s', 'nc_host')):
        res[key] = spread(walls[name])
    with open(paths['nc'], 'rb') as fa, open(host_path, 'rb') as fb:
        same = True
        while same:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            same = x == y
            if not x:
                break
    res['nc_files_identical'] = bool(same)
    # (e) the kernel and the copy, each with nothing beside it
    d_body, d_copy = ctx.empty((n,), dtype=np.uint32), ctx.empty(q.shape)
    ctx.pack_f32_be(d_q, n, d_body)
    ctx.d2d(d_copy, d_q)
    ctx.sync()
    ctx.timing_reset()
    for _ in range(a.reps):
        ctx.pack_f32_be(d_q, n, d_body)
    ms, launches = ctx.timing('pack_f32_be')
    res['e_pack_f32_be'] = {'ms': ms / launches, 'bytes': 12 * n, 'GBs': 12 * n / (ms / launches) / 1e6}
    ctx.mark_begin('d2d_copy')
    for _ in range(a.reps):
        ctx.d2d(d_copy, d_q)
    ctx.mark_end()
    ms, _ = ctx.timing('d2d_copy')
    res['e_memcpy_d2d'] = {'ms': ms / a.reps, 'bytes': 16 * n, 'GBs': 16 * n / (ms / a.reps) / 1e6}
    for arr in (d_body, d_copy, d_q):
        arr.free()
    for name in os.listdir(folder):
        os.remove(os.path.join(folder, name))
    os.rmdir(folder)
    res['b_within_110_percent_of_a'] = res['b_nc_write_s']['median'] <= 1.1 * res['a_npy_write_s']['median']
    res['b_faster_than_d'] = res['b_nc_write_s']['median'] < res['d_nc_host_route_s']['median']
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'bench_formats.json'), 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
        row = '| {} | {:.1f} MB | **{:.3f} s** ({:.3f} - {:.3f}) | {:.1f} GB/s |'
        lines = ['# Output formats from HBM: {} x {} doubles, one variable'.format(a.ncell, a.nmonths), '',
                 '`python tools/bench_formats.py --out profiles/out_formats` on {}; median (range) of {} writes after one '
                 'warm-up, the writers taking turns in one process.'.format(res['device'], a.reps), '',
                 '| writer | file | wall time | file bytes per second |', '|---|---|---|---|']
        for label, key, size in (('(a) npy, `save_npy_many` (the yardstick)', 'a_npy_write_s', 'npy_bytes'),
                                 ('(b) NetCDF from HBM, `save_nc_many`', 'b_nc_write_s', 'nc_bytes'),
                                 ('(c) MATLAB from HBM, `save_mat_many`', 'c_mat_write_s', 'mat_bytes'),
                                 ("(d) NetCDF by the host: download, `astype('>f4')`, write", 'd_nc_host_route_s', 'nc_bytes')):
            s = res[key]
            lines.append(row.format(label, res[size] / 1e6, s['median'], s['min'], s['max'], res[size] / s['median'] / 1e9))
        lines += ['', '(b) <= 1.1 x (a): **{}**; (b) faster than (d): **{}**; the files of (b) and (d) are identical: {}.'.format(
            res['b_within_110_percent_of_a'], res['b_faster_than_d'], res['nc_files_identical']), '',
            '| (e) kernel alone | time | bytes moved | rate |', '|---|---|---|---|',
            '| `xh_pack_f32_be` (8 B read + 4 B written per value) | {ms:.3f} ms | {b:.1f} MB | {GBs:.0f} GB/s |'.format(
                b=res['e_pack_f32_be']['bytes'] / 1e6, **res['e_pack_f32_be']),
            '| `xh_memcpy_d2d` of the same array (read + write) | {ms:.3f} ms | {b:.1f} MB | {GBs:.0f} GB/s |'.format(
                b=res['e_memcpy_d2d']['bytes'] / 1e6, **res['e_memcpy_d2d']), '']
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write('\n'.join(lines))


if __name__ == '__main__':
    main()
