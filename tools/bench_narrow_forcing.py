"""What an ensemble member's upload costs when its forcing is stored as float64 .npy, float32 .npy, NetCDF `float` or
NetCDF `double`, at full size (67,420 cells x 600 months, ``synth.make_world()`` defaults, 8 members, mean only).

    python tools/bench_narrow_forcing.py [--tag this] [--members 8] [--sets 2] [--reps 3] [--workdir DIR] [--out profiles/narrow_forcing]

The same forcing values (generated on the device, rounded to single precision, so that every form holds them exactly) are
written ``--sets`` times with different seeds and stored four ways; the members take the sets in turn, all from the page
cache.  Rows:
  f64_npy       pm + abcd + mrtm, eight float64 .npy per member: the path the ensemble has always had
  f32_npy       the same run, the eight arrays saved as float32
  f64_npy_hg    hargreaves + abcd + mrtm, four float64 .npy per member (the twin of the two NetCDF rows: the settings of
                the NetCDF variable names belong to that configuration)
  f32_nc        the same run, the four arrays as NetCDF-classic `float` variables
  f64_nc        ... as NetCDF-classic `double` variables
Per row, over ``--reps`` runs of ``run_ensemble(..., statistics=['mean'], member_outputs=0)`` after a warm run of two
members: the upload phase and the whole run per member (host clock around calls that end in a synchronisation; median and
range), and what ``DevicePipeline.forcing_upload`` recorded (kind and bytes host -> device per member).  Then ``xh_widen``
alone (the library's timer "widen") for the three kinds against ``xh_memcpy_d2d`` of the same array in the same process,
as GB/s of the bytes each moves.

The tool also runs on a build from before the stored-forcing path (no ``forcing_upload``, no ``xh_widen``): such a build
converts on the host and reports the times alone.  ``--tag`` names the build; the numbers go to
<out>/bench_narrow_<tag>.json, and <out>/README.md shows every tag found there side by side, with ``bench.py``'s result
lines (one per run) when they were saved beside them as <out>/bench_<tag>.json, and the text of <out>/NOTES.md."""
import argparse
import glob
import json
import os
import re
import shutil
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from xanthos_amd import _hip, run_ensemble, synth      # noqa: E402

PM = {'pm_tas': 'tas', 'pm_tmin': 'tmin', 'pm_rhs': 'rhs', 'pm_wind': 'wind', 'pm_rsds': 'rsds', 'pm_rlds': 'rlds',
      'PrecipitationFile': 'precip', 'TempMinFile': 'abcd_tmin'}
# setting -> (forcing name, setting of the NetCDF variable name, variable name)
HG = {'TemperatureFile': ('temp', 'TempVarName', 'tas'), 'DailyTemperatureRangeFile': ('dtr', 'DTRVarName', 'dtr'),
      'PrecipitationFile': ('precip', 'PrecipVarName', 'pr'), 'TempMinFile': ('abcd_tmin', 'TempMinVarName', 'tmin')}
ROWS = ('f64_npy', 'f32_npy', 'f64_npy_hg', 'f32_nc', 'f64_nc')


def spread(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'n': len(xs)}


def write_nc(path, var, values, typ):
    import scipy.io as sio
    g = sio.netcdf_file(path, 'w')
    g.createDimension('index', values.shape[0])
    g.createDimension('month', values.shape[1])
    v = g.createVariable(var, typ, ('index', 'month'))
    v[:] = values
    v.units = 'synthetic'
    g.close()


def write_sets(ctx, w, nm, nsets, folder):
    """``nsets`` forcing sets in every form; returns {row: [ {setting: path} per set ]}."""
    d_lat = ctx.upload(w.latitude)
    dev = {k: ctx.empty((w.ncell, nm)) for k in synth.FORCING_NAMES}
    paths = {row: [] for row in ROWS}
    first = None
    for k in range(nsets):
        ctx.synth_forcing(100 + k, w.ncell, nm, d_lat, dev, nan_frac=0.001)
        f32 = {name: dev[name].download().astype(np.float32) for name in synth.FORCING_NAMES}
        f32['temp'] = f32['tas']
        f32['dtr'] = f32['tas'] - f32['tmin']
        d = os.path.join(folder, 'set{}'.format(k))
        os.makedirs(d)
        for row in ROWS:
            paths[row].append({})
        for setting, name in PM.items():
            for row, dtype in (('f64_npy', np.float64), ('f32_npy', np.float32)):
                paths[row][k][setting] = os.path.join(d, '{}_{}.npy'.format(name, row[:3]))
                np.save(paths[row][k][setting], f32[name].astype(dtype))
        for setting, (name, _, var) in HG.items():
            paths['f64_npy_hg'][k][setting] = os.path.join(d, 'hg_{}_f64.npy'.format(name))
            np.save(paths['f64_npy_hg'][k][setting], f32[name].astype(np.float64))
            for row, typ in (('f32_nc', 'f4'), ('f64_nc', 'f8')):
                paths[row][k][setting] = os.path.join(d, 'hg_{}_{}.nc'.format(name, typ))
                write_nc(paths[row][k][setting], var, f32[name], typ)
        if first is None:
            first = {name: f32[name].astype(np.float64) for name in f32}
    for arr in list(dev.values()) + [d_lat]:
        arr.free()
    return paths, first


def hargreaves_ini(ini, row, files):
    """A copy of the ini for ``row`` with its four forcing settings pointing at ``files`` and the NetCDF variable names set."""
    text = open(ini).read()
    for setting, (_, varname, var) in HG.items():
        text, n = re.subn(r'(?m)^{} = .*$'.format(setting), '{} = {}\n{} = {}'.format(setting, files[setting], varname, var), text)
        assert n == 1, setting
    out = ini.replace('.ini', '_{}.ini'.format(row))
    with open(out, 'w') as fh:
        fh.write(text)
    return out


def widen_bench(ctx, n, reps):
    """xh_widen of n values per kind, and xh_memcpy_d2d of n doubles, each alone: ms and GB/s of the bytes moved."""
    out = {}
    rng = np.random.default_rng(3)
    values = rng.gamma(0.7, 40.0, n).astype(np.float32)
    d_dst, d_copy = ctx.empty((n,)), ctx.empty((n,))
    for label, kind, raw, moved in (('f32', _hip.XH_SRC_F32_LE, values, 12), ('f32be', _hip.XH_SRC_F32_BE, values.astype('>f4'), 12),
                                    ('f64be', _hip.XH_SRC_F64_BE, values.astype('>f8'), 16)):
        d_src = ctx.upload(raw.view(np.uint8), dtype=np.uint8)
        ctx.widen(d_src, kind, n, d_dst)                   # warm
        ctx.sync()
        ctx.timing_reset()
        for _ in range(reps):
            ctx.widen(d_src, kind, n, d_dst)
        ms, launches = ctx.timing('widen')
        assert np.array_equal(d_dst.download(), values.astype(np.float64))
        out[label] = {'ms': ms / launches, 'bytes': moved * n, 'GBs': moved * n / (ms / launches) / 1e6}
        d_src.free()
    ctx.d2d(d_copy, d_dst)
    ctx.sync()
    ctx.mark_begin('d2d_copy')
    for _ in range(reps):
        ctx.d2d(d_copy, d_dst)
    ctx.mark_end()
    ms, _ = ctx.timing('d2d_copy')
    out['memcpy_d2d'] = {'ms': ms / reps, 'bytes': 16 * n, 'GBs': 16 * n / (ms / reps) / 1e6}
    d_dst.free()
    d_copy.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tag', default='this', help="names the build in the output ('this', 'parent')")
    ap.add_argument('--members', type=int, default=8)
    ap.add_argument('--sets', type=int, default=2, help='distinct forcing sets on disk; the members take them in turn')
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rows', default=','.join(ROWS))
    ap.add_argument('--spinup', type=int, default=120, help='runoff and routing spin-up months')
    ap.add_argument('--small', action='store_true', help='a 900-cell world: a rehearsal of the tool, not a measurement')
    ap.add_argument('--workdir', default=None, help='where the input trees go (default: a temporary directory)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'narrow_forcing'))
    ap.add_argument('--readme-only', action='store_true', help='rewrite <out>/README.md from the json files there')
    a = ap.parse_args()
    if a.readme_only:
        write_readme(a.out)
        return
    if a.workdir is None:
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix='xh_bench_narrow_')
    ctx = _hip.get_context(0)
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7) if a.small else synth.make_world()
    nm, S = a.months, a.members
    y0, y1 = 1961, 1961 + nm // 12 - 1
    result = {'tag': a.tag, 'device': ctx.name(), 'stored_path': hasattr(_hip.Context, 'widen'),
              'workload': '{} cells x {} months, spin-ups {} / {}, {} members over {} forcing sets, mean only, '
                          '{} runs per row'.format(w.ncell, nm, a.spinup, a.spinup, S, a.sets, a.reps), 'rows': {}}
    shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.workdir)
    paths, first = write_sets(ctx, w, nm, a.sets, a.workdir)
    pm_ini = synth.write_example(os.path.join(a.workdir, 'pm'), w, first, y0, y1, runoff_spinup=a.spinup, routing_spinup=a.spinup,
                                 output_vars=('q', 'avgchflow'), output_format=4)
    hg_ini = synth.write_hgm_example(os.path.join(a.workdir, 'hg'), w, first, y0, y1, runoff='abcd', runoff_spinup=a.spinup,
                                     routing_spinup=a.spinup, output_vars=('q', 'avgchflow'))
    for row in a.rows.split(','):
        ini = pm_ini if row in ('f64_npy', 'f32_npy') else hargreaves_ini(hg_ini, row, paths[row][0])
        members = [('m{:02d}'.format(k), paths[row][k % a.sets]) for k in range(S)]
        kw = dict(statistics=['mean'], member_outputs=0)
        run_ensemble(ini, members=members[:2], **kw)          # warm: contexts, rings, the page cache
        upload, total, sent = [], [], None
        for _ in range(a.reps):
            t = time.perf_counter()
            res = run_ensemble(ini, members=members, **kw)
            total.append(1e3 * (time.perf_counter() - t) / S)
            upload.append(1e3 * float(np.mean(res.timings['upload'])))
            sent = getattr(res, 'forcing_upload', None)
        entry = {'upload_ms_per_member': spread(upload), 'total_ms_per_member': spread(total),
                 'kernels_ms_per_member': 1e3 * float(np.mean(res.timings['kernels']))}
        if sent:
            entry['kinds'] = sorted({v[0] for v in sent[0].values()})
            entry['bytes_per_member'] = int(sum(v[1] for v in sent[0].values()))
        result['rows'][row] = entry
        print(row, json.dumps(entry), flush=True)
    if result['stored_path']:
        result['widen'] = widen_bench(ctx, w.ncell * nm, 5)
    shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_narrow_{}.json'.format(a.tag)), 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    write_readme(a.out)
    print(json.dumps(result))


def write_readme(out):
    runs = {}
    for path in sorted(glob.glob(os.path.join(out, 'bench_narrow_*.json'))):
        with open(path) as fh:
            r = json.load(fh)
        runs[r['tag']] = r
    tags = sorted(runs, key=lambda t: (t != 'parent', t))
    lines = ['# Forcing uploaded as stored: measurements', '', 'Written by `tools/bench_narrow_forcing.py`.', '']
    for t in tags:
        lines.append('- `{}`: {}; {}; forcing {}.'.format(t, runs[t]['device'], runs[t]['workload'],
                                                         'sent as stored and widened in HBM' if runs[t]['stored_path']
                                                         else 'converted to float64 on the host'))
    head = '| row | ' + ' | '.join('{}: upload | {}: whole run'.format(t, t) for t in tags) + ' | bytes sent per member | kinds |'
    lines += ['', 'Milliseconds per member, median (range) over the runs; upload = the upload phase of `run_ensemble` (reading, '
              'any host conversion, the copy, the widen), whole run = wall time of the call / members.', '', head,
              '|---|' + '---|---|' * len(tags) + '---|---|']
    cell = lambda s: '{:.1f} ({:.1f} - {:.1f})'.format(s['median'], s['min'], s['max'])      # noqa: E731
    for row in ROWS:
        if not any(row in runs[t]['rows'] for t in tags):
            continue
        cols, extra = [], ('', '')
        for t in tags:
            e = runs[t]['rows'].get(row)
            cols += [cell(e['upload_ms_per_member']), cell(e['total_ms_per_member'])] if e else ['', '']
            if e and 'bytes_per_member' in e:
                extra = ('{:.0f} MB'.format(e['bytes_per_member'] / 1e6), ', '.join(e['kinds']))
        lines.append('| {} | '.format(row) + ' | '.join(cols) + ' | {} | {} |'.format(*extra))
    for t in tags:
        k = runs[t].get('widen')
        if k:
            lines += ['', '| `{}`: kernel alone, {:,} values | time | bytes moved | rate |'.format(t, k['memcpy_d2d']['bytes'] // 16),
                      '|---|---|---|---|']
            for label, text in (('f32', '`xh_widen` float32 (4 B read + 8 B written per value)'),
                                ('f32be', '`xh_widen` big-endian float32'), ('f64be', '`xh_widen` big-endian float64 (8 + 8)'),
                                ('memcpy_d2d', '`xh_memcpy_d2d` of the doubles (read + write)')):
                lines.append('| {} | {:.3f} ms | {:.1f} MB | {:.0f} GB/s |'.format(text, k[label]['ms'], k[label]['bytes'] / 1e6,
                                                                                 k[label]['GBs']))
    bench = []
    for t in tags:
        path = os.path.join(out, 'bench_{}.json'.format(t))
        if os.path.isfile(path):
            with open(path) as fh:
                steps = [json.loads(line)['ms_per_step'] for line in fh.read().strip().splitlines()]
            bench.append('| {} | {} |'.format(t, ', '.join('{:.2f}'.format(ms) for ms in steps)))
    if bench:
        lines += ['', '`python bench.py --gpus 1 --steps 5 --warmup 1` (float64 forcing generated on the device: the path this change '
                  'leaves alone), the builds taking turns:', '', '| build | ms per step, run by run |', '|---|---|'] + bench
    notes = os.path.join(out, 'NOTES.md')
    if os.path.isfile(notes):
        with open(notes) as fh:
            lines += ['', fh.read().rstrip()]
    with open(os.path.join(out, 'README.md'), 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
