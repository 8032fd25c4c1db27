"""The gridded map of one monthly variable at the 0.5-degree grid size: 67,420 cells x 600 months in HBM -> [600, 360, 720].

    python tools/bench_gridded.py [--reps 5] [--out profiles/gridded]

All in one process, on the synthetic world of ``synth.make_world()`` (67,420 cells on 360 x 720):
  (1) xh_grid_pack_f32_be alone, from the library's timer "grid_pack", as GB/s of its floor -- 8 ncell ncols bytes read,
      4 nslots ncols written, the table once per time tile of 64 -- next to xh_pack_f32_be (the per-cell body: 12 bytes
      per value) and xh_memcpy_d2d of the same array (16 bytes per value)
  (2) wall time of the map's file (Context.save_grid_nc_many: header, kernel, xh_download_files) against the host path
      to the same file: download, numpy scatter into a '>f4' cube of fill values, header + bytes in one write.  The two
      files are compared byte for byte.
  (3) the per-cell NetCDF file of the same variable (OutputFormat 0, save_nc_many), for scale.
Wall times: the writers take turns, the first round is dropped, median and range of the rest.  With --out the table goes
to <out>/README.md, the numbers to <out>/bench_gridded.json.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))


def spread(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'n': len(xs)}


def main():
    from xanthos_amd import _hip, synth
    from xanthos_amd.data_writer import formats, gridded
    ap = argparse.ArgumentParser()
    ap.add_argument('--nmonths', type=int, default=600)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='900 cells on 36 x 72 (a check of the tool, not a measurement)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7) if a.small else synth.make_world()
    grid = gridded.GridMap(w.coords, w.nrow, w.ncol)
    ncell, nt, nslots = w.ncell, a.nmonths, grid.nslots
    rng = np.random.default_rng(1)
    q = rng.gamma(0.7, 40.0, (ncell, nt))                       # like monthly runoff in mm
    q[rng.random(q.shape) < 0.01] = np.nan
    d_q = ctx.upload(q)
    table = grid.device_table(ctx)
    folder = tempfile.mkdtemp(prefix='bench_gridded_')
    days, units = gridded.time_axis(1971, nt, 0)
    header = gridded.grid_nc_header('q', 'mmpermonth', days, units, grid, title='bench')
    paths = {k: os.path.join(folder, k + '.nc') for k in ('grid', 'grid_host', 'cell')}

    def host_route():
        data = d_q.download()
        cube = np.full((nt, nslots), gridded.FILL, '>f4')
        with np.errstate(over='ignore'):
            v = data.T.astype('>f4')
        v[np.isnan(data.T)] = gridded.FILL
        cube[:, grid.slot_of_cell] = v
        with open(paths['grid_host'], 'wb') as fh:
            fh.write(header)
            fh.write(memoryview(cube).cast('B'))

    runs = (('grid', lambda: ctx.save_grid_nc_many([(paths['grid'], header, d_q, grid)])),
            ('grid_host', host_route),
            ('cell', lambda: ctx.save_nc_many([(paths['cell'], formats.nc_header(ncell, nt, 0, 'mmpermonth', 'q'), d_q)])))
    walls = {name: [] for name, _ in runs}
    for rep in range(a.reps + 1):
        for name, run in runs:
            ctx.sync()
            t = time.perf_counter()
            run()
            dt = time.perf_counter() - t
            if rep:
                walls[name].append(dt)
    res = {'device': ctx.name(), 'ncell': ncell, 'nmonths': nt, 'ngridrow': w.nrow, 'ngridcol': w.ncol,
           'array_bytes': int(q.nbytes), 'land_fraction': ncell / nslots,
           'ocean_tiles_of_64_slots': int((grid.cell_of_slot[:nslots // 64 * 64].reshape(-1, 64).max(axis=1) < 0).sum()),
           'tiles_of_64_slots': (nslots + 63) // 64}
    for k, p in paths.items():
        res[k + '_bytes'] = os.path.getsize(p)
    for key, name in (('grid_write_s', 'grid'), ('grid_host_route_s', 'grid_host'), ('cell_nc_write_s', 'cell')):
        res[key] = spread(walls[name])
    with open(paths['grid'], 'rb') as fa, open(paths['grid_host'], 'rb') as fb:
        same = True
        while same:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            same = x == y
            if not x:
                break
    res['grid_files_identical'] = bool(same)
    # (1) the kernels and the copy, each with nothing beside it
    d_body, d_cell, d_copy = ctx.empty((nt * nslots,), dtype=np.uint32), ctx.empty((q.size,), dtype=np.uint32), ctx.empty(q.shape)
    ctx.grid_pack_f32_be(d_q, table, nslots, grid.fill_bits, d_body)
    ctx.pack_f32_be(d_q, q.size, d_cell)
    ctx.d2d(d_copy, d_q)
    ctx.sync()
    ctx.timing_reset()
    for _ in range(a.reps):
        ctx.grid_pack_f32_be(d_q, table, nslots, grid.fill_bits, d_body)
    for _ in range(a.reps):
        ctx.pack_f32_be(d_q, q.size, d_cell)
    floor = 8 * q.size + 4 * nslots * nt + 4 * nslots * ((nt + 63) // 64)
    for key, name, nbytes in (('grid_pack', 'grid_pack', floor), ('pack_f32_be', 'pack_f32_be', 12 * q.size)):
        ms, launches = ctx.timing(name)
        res[key] = {'ms': ms / launches, 'bytes': nbytes, 'GBs': nbytes / (ms / launches) / 1e6}
    ctx.mark_begin('d2d_copy')
    for _ in range(a.reps):
        ctx.d2d(d_copy, d_q)
    ctx.mark_end()
    ms, _ = ctx.timing('d2d_copy')
    res['memcpy_d2d'] = {'ms': ms / a.reps, 'bytes': 16 * q.size, 'GBs': 16 * q.size / (ms / a.reps) / 1e6}
    for arr in (d_body, d_cell, d_copy, d_q):
        arr.free()
    for name in os.listdir(folder):
        os.remove(os.path.join(folder, name))
    os.rmdir(folder)
    res['grid_pack_rate_over_copy_rate'] = res['grid_pack']['GBs'] / res['memcpy_d2d']['GBs']
    res['grid_write_over_host_route'] = res['grid_write_s']['median'] / res['grid_host_route_s']['median']
    res['grid_write_over_cell_nc_write'] = res['grid_write_s']['median'] / res['cell_nc_write_s']['median']
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'bench_gridded.json'), 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
        krow = '| {} | {:.3f} ms | {:.1f} MB | {:.0f} GB/s |'
        wrow = '| {} | {:.1f} MB | **{:.3f} s** ({:.3f} - {:.3f}) | {:.2f} GB/s |'
        lines = ['# Gridded maps from HBM: {} cells x {} months -> [{}, {}, {}]'.format(ncell, nt, nt, w.nrow, w.ncol), '',
                 '`python tools/bench_gridded.py --out profiles/gridded` on {}; {:.0%} of the {} slots hold a cell, {} of the '
                 '{} tiles of 64 slots hold none.'.format(res['device'], res['land_fraction'], nslots,
                                                         res['ocean_tiles_of_64_slots'], res['tiles_of_64_slots']), '',
                 '| kernel alone (mean of {} launches) | time | bytes at the least | rate |'.format(a.reps), '|---|---|---|---|',
                 krow.format('`xh_grid_pack_f32_be` (8 B read per value, 4 B written per slot and month, the table per time '
                             'tile)', res['grid_pack']['ms'], res['grid_pack']['bytes'] / 1e6, res['grid_pack']['GBs']),
                 krow.format('`xh_pack_f32_be`, the per-cell body (8 B read + 4 B written per value)', res['pack_f32_be']['ms'],
                             res['pack_f32_be']['bytes'] / 1e6, res['pack_f32_be']['GBs']),
                 krow.format('`xh_memcpy_d2d` of the same array (read + write)', res['memcpy_d2d']['ms'],
                             res['memcpy_d2d']['bytes'] / 1e6, res['memcpy_d2d']['GBs']), '',
                 'The gather-transpose runs at **{:.2f} x** the copy\'s rate over its floor.'.format(
                     res['grid_pack_rate_over_copy_rate']), '',
                 '| file of one monthly variable (median and range of {} writes after a warm-up) | file | wall time | file '
                 'bytes per second |'.format(a.reps), '|---|---|---|---|']
        for label, key, size in (('map from HBM, `save_grid_nc_many`', 'grid_write_s', 'grid_bytes'),
                                 ('map by the host: download, numpy scatter into a `>f4` cube, write', 'grid_host_route_s',
                                  'grid_host_bytes'),
                                 ('per-cell NetCDF from HBM, `save_nc_many` (for scale)', 'cell_nc_write_s', 'cell_bytes')):
            s = res[key]
            lines.append(wrow.format(label, res[size] / 1e6, s['median'], s['min'], s['max'], res[size] / s['median'] / 1e9))
        lines += ['', 'The map from HBM takes **{:.2f} x** the host path\'s time and {:.2f} x the per-cell file\'s ({:.1f} x its '
                  'bytes); the two maps are identical: {}.'.format(
                      res['grid_write_over_host_route'], res['grid_write_over_cell_nc_write'],
                      res['grid_bytes'] / res['cell_bytes'], res['grid_files_identical']), '']
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write('\n'.join(lines))


if __name__ == '__main__':
    main()
