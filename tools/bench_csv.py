"""The csv writer at the 0.5-degree grid size: one monthly variable, 67,420 cells x 600 months in HBM.

    python tools/bench_csv.py [--reps 5] [--host-reps 1] [--out profiles/csv_writer/bench_csv.json]

Times (wall clock around calls that return when the file is complete; the first repetition warms code objects, slots and
the page cache and is dropped; median and range of the rest):
  (a) host_loop   what OutWriter.write() did before the device formatter: download, then one repr(float(v)) per value
  (b) csv         OutWriter.write() of the same variable as it is now (header on the host, xh_csv_write_many behind it)
  (c) npy         OutWriter.write() with OutputFormat 4 (save_npy_many)
and the phases of (b) on their own: the format kernels (the library's HIP-event timers "csv_measure" and "csv_emit" of the
timed runs), the text device -> page-locked host (one copy of the whole text), and write() of that text from host memory.
The format kernels are also timed with nothing beside them (xh_csv_format of the whole array).  The files of (a) and (b)
are compared byte for byte.  XH_LIBRARY=<a library of `make expcsv`> times another layout of the kernels.
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


def host_loop(path, dev, col_names):
    """out_writer.py's csv branch before xh_csv_write (kept by it for tables with names)."""
    data = dev.download()
    fmt = lambda v: '' if v != v else repr(float(v))
    with open(path, 'w') as fh:
        fh.write('id,' + ','.join(col_names) + '\n')
        for i, row in zip(range(1, data.shape[0] + 1), data):
            fh.write(str(i) + ',' + ','.join(fmt(v) for v in row) + '\n')


def main():
    from xanthos_amd import _hip
    from xanthos_amd.data_writer.out_writer import OutWriter
    ap = argparse.ArgumentParser()
    ap.add_argument('--ncell', type=int, default=67420)
    ap.add_argument('--nmonths', type=int, default=600)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    rng = np.random.default_rng(1)
    q = rng.gamma(0.7, 40.0, (a.ncell, a.nmonths))             # like monthly runoff in mm
    q[rng.random(q.shape) < 0.01] = 0.0
    d_q = ctx.upload(q)
    folder = tempfile.mkdtemp(prefix='bench_csv_')
    years = a.nmonths // 12

    def writer(fmt):
        s = SimpleNamespace(output_vars=['q'], ProjectName='bench', OutputFolder=folder, OutputFormat=fmt, OutputUnit=0,
                            OutputInYear=0, StartYear=1971, EndYear=1970 + years, device=0)
        return OutWriter(s, np.ones(a.ncell), {'q': d_q})

    res = {'device': ctx.name(), 'library': os.path.basename(_hip.LIB_PATH), 'ncell': a.ncell, 'nmonths': a.nmonths, 'array_bytes': int(q.nbytes)}
    csv_path = os.path.join(folder, 'q_mmpermonth_bench.csv')
    kernels = {'csv_measure': [], 'csv_emit': []}
    walls = {'csv': [], 'npy': []}
    for rep in range(a.reps + 1):                                # alternating, the first of each a warm-up
        for name, fmt in (('csv', 1), ('npy', 4)):
            w = writer(fmt)
            ctx.sync()
            ctx.timing_reset()
            t = time.perf_counter()
            w.write()
            dt = time.perf_counter() - t
            if rep:
                walls[name].append(dt)
                if name == 'csv':
                    for k in kernels:
                        kernels[k].append(ctx.timing(k)[0] / 1e3)
    res['csv_bytes'] = os.path.getsize(csv_path)
    res['npy_bytes'] = os.path.getsize(os.path.join(folder, 'q_mmpermonth_bench.npy'))
    res['b_csv_write_s'] = spread(walls['csv'])
    res['c_npy_write_s'] = spread(walls['npy'])
    res['b_phase_format_kernels_s'] = {k: spread(v) for k, v in kernels.items()}
    # the other two phases of (b), each on its own: the text of the whole array in HBM -> page-locked host -> file
    nrows, ncols = d_q.shape
    cap = res['csv_bytes']
    d_text, d_off = ctx.empty((cap,), dtype=np.uint8), ctx.empty((nrows + 1,), dtype=np.int64)
    alone = {'csv_measure': [], 'csv_emit': []}                  # the kernels with nothing beside them: the whole text at once
    for rep in range(a.reps + 1):
        ctx.sync()
        ctx.timing_reset()
        ctx._check(_hip.lib().xh_csv_format(ctx.handle, d_q.ptr, nrows, ncols, 1, d_text.ptr, cap, d_off.ptr))
        if rep:
            for k in alone:
                alone[k].append(ctx.timing(k)[0] / 1e3)
    res['format_whole_array_kernels_s'] = {k: spread(v) for k, v in alone.items()}
    pinned = ctx.pinned((cap,), dtype=np.uint8)
    copies, writes = [], []
    raw = os.path.join(folder, 'text.raw')
    for rep in range(a.reps + 1):
        ctx.sync()
        t = time.perf_counter()
        d_text.download(out=pinned)
        dt = time.perf_counter() - t
        t = time.perf_counter()
        with open(raw, 'wb') as fh:
            fh.write(memoryview(pinned))
        dw = time.perf_counter() - t
        if rep:
            copies.append(dt)
            writes.append(dw)
    res['b_phase_text_to_host_s'] = spread(copies)
    res['b_phase_file_write_s'] = spread(writes)
    header = len(open(csv_path, 'rb').readline())
    res['text_bytes'] = int(d_off.download()[-1])
    assert res['text_bytes'] + header == res['csv_bytes']
    ctx.free_pinned(pinned)
    d_text.free()
    d_off.free()
    steps = ['{}{:02}'.format(1971 + y, m) for y in range(years) for m in range(1, 13)]
    host_path = os.path.join(folder, 'host_loop.csv')
    times = []
    for rep in range(a.host_reps):
        t = time.perf_counter()
        host_loop(host_path, d_q, steps)
        times.append(time.perf_counter() - t)
    if times:
        res['a_host_loop_write_s'] = spread(times)
        same = os.path.getsize(host_path) == res['csv_bytes']
        if same:
            with open(host_path, 'rb') as fa, open(csv_path, 'rb') as fb:
                while same:
                    x, y = fa.read(1 << 24), fb.read(1 << 24)
                    same = x == y
                    if not x:
                        break
        res['files_identical'] = bool(same)
    for n in os.listdir(folder):
        os.remove(os.path.join(folder, n))
    os.rmdir(folder)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
