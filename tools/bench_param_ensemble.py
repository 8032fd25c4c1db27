"""The parameter ensemble (members that vary the ABCD table on resident forcing) against a loop of single runs, and the
skill kernel against a device copy, at full size (67,420 cells x 600 months, ``synth.make_world()`` defaults, pm_abcd_mrtm,
spin-ups 120 / 120, S = 8 parameter tables inside the calibration's box).

    python tools/bench_param_ensemble.py [--members 8] [--months 600] [--workdir DIR]      # writes the JSON and README
    python tools/bench_param_ensemble.py --kernel-only                                     # (c) alone

(a) baseline: milliseconds per member of a warm loop of ``Xanthos(ini).execute({'calib_file': table_k})`` over the members
    -- the path a user has without the member key ``abcd_pars`` (unchanged by it);
(b) ``run_ensemble`` with ``abcd_pars`` members, resident (one upload, one PET), overlapped and one after the other: npy
    member outputs without statistics; member_outputs = 0 with the mean; the same with ``observed`` (the KGE table);
(c) ``xh_basin_kge`` on one Q array with all 235 basins observed: time of the library's ``basin_kge`` timer (both kernels),
    GB/s of its floor -- one read of Q, n x 8 B -- and ``xh_memcpy_d2d`` of one array (2 x n x 8 B) in the same process as
    the bandwidth yardstick.
Results: profiles/param_ensemble/bench_param_ensemble.json and the table in profiles/param_ensemble/README.md."""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from xanthos_amd import Xanthos, _hip, run_ensemble, synth      # noqa: E402

LB = 1e-4
BOX_LO, BOX_HI = np.full(5, LB), np.array([1 - LB, 8 - LB, 1 - LB, 1 - LB, 1 - LB])


def parameter_tables(pars, S):
    """S tables: the world's own, then each column scaled by a factor of its own per member, kept inside the box."""
    tables = [np.asarray(pars, dtype=np.float64)]
    for k in range(1, S):
        f = 1.0 + 0.25 * np.sin(1.7 * k + np.arange(5))
        tables.append(np.clip(pars * f, BOX_LO, BOX_HI))
    return tables


def skill_tables(w, nmonths, seed=5):
    basins = sorted(set(int(b) for b in w.basin_ids))
    cells = [np.flatnonzero(w.basin_ids == b) for b in basins]
    start = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    obs = np.random.default_rng(seed).uniform(0.5, 5.0, size=(len(basins), nmonths))
    return basins, start, np.concatenate(cells).astype(np.int32), obs


def kernel_bench(ctx, w, nmonths, reps=10):
    ncell, n = w.ncell, w.ncell * nmonths
    d_lat = ctx.upload(w.latitude)
    q, copy = ctx.empty((ncell, nmonths)), ctx.empty((ncell, nmonths))
    ctx.synth_forcing(1, ncell, nmonths, d_lat, {'tas': q})        # a monthly array of the benchmark world (values only matter as bytes)
    basins, start, cells, obs = skill_tables(w, nmonths)
    nb = len(basins)
    d = [ctx.upload(start, dtype=np.int64), ctx.upload(cells, dtype=np.int32), ctx.upload(w.area), ctx.upload(obs),
         ctx.empty((nb, nmonths)), ctx.empty((nb,))]
    out = {'basins': nb, 'cells_per_basin_max': int(np.diff(start).max()), 'cells_per_basin_mean': float(np.diff(start).mean())}
    for tag, area in (('km3_per_mth', d[2]), ('mm_per_mth', None)):
        ctx.basin_kge(ncell, nmonths, nb, d[0], d[1], q, area, d[3], d[5], series=d[4])      # warm
        ctx.sync()
        ctx.timing_reset()
        for _ in range(reps):
            ctx.basin_kge(ncell, nmonths, nb, d[0], d[1], q, area, d[3], d[5], series=d[4])
        ctx.sync()
        ms, launches = ctx.timing('basin_kge')
        out[tag] = {'ms': ms / launches, 'floor_bytes': n * 8, 'GBs': n * 8 / (ms / launches) / 1e6}
    ctx.d2d(copy, q)
    ctx.sync()
    ctx.mark_begin('d2d_copy')
    for _ in range(reps):
        ctx.d2d(copy, q)
    ctx.mark_end()
    ms, _ = ctx.timing('d2d_copy')
    out['memcpy_d2d'] = {'ms': ms / reps, 'bytes': 2 * n * 8, 'GBs': 2 * n * 8 / (ms / reps) / 1e6}
    for a in d + [q, copy, d_lat]:
        a.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=8)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--workdir', default=None, help='where the input tree and the outputs go (default: a temporary directory)')
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'param_ensemble'))
    a = ap.parse_args()
    if a.workdir is None:
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix='xh_bench_param_ensemble_')
    ctx = _hip.get_context(0)
    w = synth.make_world()
    nm, S = a.months, a.members
    result = {'device': ctx.name(), 'workload': '{} cells x {} months, pm_abcd_mrtm, spin-ups 120 / 120, {} parameter tables'
              .format(w.ncell, nm, S)}
    result['skill_kernel'] = kernel_bench(ctx, w, nm)
    if not a.kernel_only:
        d_lat = ctx.upload(w.latitude)
        dev = {k: ctx.empty((w.ncell, nm)) for k in synth.FORCING_NAMES}
        ctx.synth_forcing(100, w.ncell, nm, d_lat, dev, nan_frac=0.001)
        forcing = {name: dev[name].download() for name in synth.FORCING_NAMES}
        for arr in list(dev.values()) + [d_lat]:
            arr.free()
        shutil.rmtree(a.workdir, ignore_errors=True)
        os.makedirs(a.workdir)
        ini = synth.write_example(a.workdir, w, forcing, 1961, 1961 + nm // 12 - 1, runoff_spinup=120, routing_spinup=120,
                                  output_vars=('q', 'avgchflow'), output_format=4)
        del forcing
        out_dir = os.path.join(a.workdir, 'output', 'pm_abcd_mrtm_synth')
        tables = parameter_tables(w.abcd_pars, S)
        members = [('p{:02d}'.format(k), {'abcd_pars': t}) for k, t in enumerate(tables)]
        basins, _, _, obs = skill_tables(w, nm)
        obs_rows = np.array([[b, 0.0, 0.0, v] for b, row in zip(basins, obs) for v in row])
        # (a) the loop of single runs, warm (one run first)
        Xanthos(ini).execute({'calib_file': tables[0], 'OutputFolder': os.path.join(out_dir, 'warm')})
        t = time.perf_counter()
        for (name, _), table in zip(members, tables):
            Xanthos(ini).execute({'calib_file': table, 'OutputFolder': os.path.join(out_dir, 'single_' + name)})
        base_ms = 1e3 * (time.perf_counter() - t) / S
        result['baseline_loop_ms_per_member'] = base_ms
        # (b) the resident parameter ensemble
        skill = dict(observed=obs_rows, obs_unit='km3_per_mth')
        runs = {}
        for tag, kw in (('npy_outputs', dict(member_outputs=1)), ('stats_only', dict(statistics=['mean'], member_outputs=0)),
                        ('stats_only_with_kge', dict(statistics=['mean'], member_outputs=0, **skill))):
            for overlap in (True, False):
                run_ensemble(ini, members=members[:2], overlap=overlap, **kw)          # warm: contexts, rings
                t = time.perf_counter()
                res = run_ensemble(ini, members=members, overlap=overlap, **kw)
                ms = 1e3 * (time.perf_counter() - t) / S
                assert all(not u for u in res.forcing_upload[1:])                      # resident: one upload
                runs['{}_{}'.format(tag, 'overlapped' if overlap else 'serial')] = {
                    'ms_per_member': ms, 'ratio_to_baseline': ms / base_ms,
                    'upload_ms_once': 1e3 * res.timings['upload'][0],
                    'phases_ms_per_member': {k: 1e3 * float(np.mean(res.timings[k][1:])) for k in ('kernels', 'post', 'write')},
                    'first_member_kernels_ms': 1e3 * res.timings['kernels'][0],
                    'statistics_ms': 1e3 * res.timings['statistics']}
        result['ensemble'] = runs
        shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.out, exist_ok=True)
    name = 'bench_param_ensemble_kernel.json' if a.kernel_only else 'bench_param_ensemble.json'
    with open(os.path.join(a.out, name), 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    if not a.kernel_only:
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write(readme(result))
    print(json.dumps(result))


def readme(r):
    k = r['skill_kernel']
    lines = ['# Parameter ensemble: measurements', '', 'Written by `tools/bench_param_ensemble.py` on {}.'.format(r['device']), '',
             'Workload: {}.  The forcing is uploaded once and PET is computed once (with the first member); the '
             'per-member figures of (b) are wall time of the whole call divided by the members, the phases are means over '
             'the members after the first.'.format(r['workload']), '',
             '| path | ms per member | ratio to the loop of single runs |', '|---|---|---|',
             "| (a) warm loop of `Xanthos(ini).execute({{'calib_file': table_k}})`, npy outputs | {:.1f} | 1.00 |".format(
                 r['baseline_loop_ms_per_member'])]
    for tag, v in sorted(r['ensemble'].items()):
        lines.append('| (b) `run_ensemble` with `abcd_pars`, {} | {:.1f} | {:.2f} |'.format(
            tag.replace('_', ' '), v['ms_per_member'], v['ratio_to_baseline']))
    lines += ['', '| phase (ms) | ' + ' | '.join(sorted(r['ensemble'])) + ' |', '|---|' + '---|' * len(r['ensemble'])]
    for label, get in (('upload, once', lambda v: v['upload_ms_once']), ('kernels, first member (with PET)', lambda v: v['first_member_kernels_ms']),
                       ('kernels per later member', lambda v: v['phases_ms_per_member']['kernels']),
                       ('post per later member', lambda v: v['phases_ms_per_member']['post']),
                       ('write per later member', lambda v: v['phases_ms_per_member']['write']),
                       ('statistics, once', lambda v: v['statistics_ms'])):
        lines.append('| {} | '.format(label) + ' | '.join('{:.1f}'.format(get(r['ensemble'][t])) for t in sorted(r['ensemble'])) + ' |')
    lines += ['', '| (c) skill kernel, {} basins (largest {} cells) | ms | GB | GB/s |'.format(k['basins'], k['cells_per_basin_max']),
              '|---|---|---|---|']
    for tag in ('km3_per_mth', 'mm_per_mth'):
        lines.append('| `xh_basin_kge`, {} (floor: one read of Q) | {:.3f} | {:.2f} | {:.0f} |'.format(
            tag, k[tag]['ms'], k[tag]['floor_bytes'] / 1e9, k[tag]['GBs']))
    lines.append('| `xh_memcpy_d2d` of one array (read + write) | {:.3f} | {:.2f} | {:.0f} |'.format(
        k['memcpy_d2d']['ms'], k['memcpy_d2d']['bytes'] / 1e9, k['memcpy_d2d']['GBs']))
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    main()
