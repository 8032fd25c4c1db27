"""The ensemble run against a loop of single runs, and the statistics kernel against a device copy, at full size
(67,420 cells x 600 months, ``synth.make_world()`` defaults, pm_abcd_mrtm, S = 8 members of pinned in-memory forcing).

    python tools/bench_ensemble.py [--members 8] [--months 600] [--workdir DIR]      # (a) + (b) + (c), writes the JSON and README
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_ensemble.py --kernel-only      # (c) alone, for the kernel trace

(a) baseline: milliseconds per member of a warm loop of ``Xanthos(ini).execute(args_k)`` over the members -- the path a
    user has without this module;
(b) ``run_ensemble`` per member, overlapped and one after the other, with member_outputs = 0 (mean only) and with npy
    member outputs (no statistics);
(c) ``xh_ens_stats`` for mean + std + q10 / q50 / q90 over S = 8 and S = 32 monthly arrays: kernel time (HIP events of the
    library's ``ens_stats`` timer), achieved GB/s of its algorithmic traffic (S + outputs) x n x 8 B, and
    ``xh_memcpy_d2d`` of one array (2 x n x 8 B) in the same process as the machine's bandwidth yardstick.
Results: profiles/ensemble/bench_ensemble.json and the table in profiles/ensemble/README.md."""
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

SETTINGS = {'pm_tas': 'tas', 'pm_tmin': 'tmin', 'pm_rhs': 'rhs', 'pm_wind': 'wind', 'pm_rsds': 'rsds', 'pm_rlds': 'rlds',
            'PrecipitationFile': 'precip', 'TempMinFile': 'abcd_tmin'}
STATS = ('mean', 'std')
QUANTILES = (0.1, 0.5, 0.9)


def kernel_bench(ctx, ncell, nmonths, counts=(8, 32), reps=5):
    n = ncell * nmonths
    out = {}
    d_lat = ctx.upload(synth.make_world().latitude)

    def fresh(seed):                                      # a monthly array of its own (temperature of the benchmark world)
        arr = ctx.empty((ncell, nmonths))
        ctx.synth_forcing(seed, ncell, nmonths, d_lat, {'tas': arr})
        return arr
    base = fresh(1)
    outs = [ctx.empty((ncell, nmonths)) for _ in range(len(STATS) + len(QUANTILES))]
    copy = ctx.empty((ncell, nmonths))
    for S in counts:
        members = [base] + [fresh(10 + j) for j in range(1, S)]           # S distinct arrays: nothing is served twice from a cache
        ctx.ens_stats(n, members, STATS, QUANTILES, outs)                  # warm
        ctx.sync()
        ctx.timing_reset()
        for _ in range(reps):
            ctx.ens_stats(n, members, STATS, QUANTILES, outs)
        ms, launches = ctx.timing('ens_stats')
        traffic = (S + len(outs)) * n * 8
        out['S{}'.format(S)] = {'kernel_ms': ms / launches, 'algorithmic_bytes': traffic,
                                'GBs': traffic / (ms / launches) / 1e6}
        for m in members[1:]:
            m.free()
    ctx.d2d(copy, base)
    ctx.sync()
    ctx.mark_begin('d2d_copy')
    for _ in range(reps):
        ctx.d2d(copy, base)
    ctx.mark_end()
    ms, _ = ctx.timing('d2d_copy')
    out['memcpy_d2d'] = {'ms': ms / reps, 'bytes': 2 * n * 8, 'GBs': 2 * n * 8 / (ms / reps) / 1e6}
    for a in outs + [copy, base, d_lat]:
        a.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=8)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--workdir', default=None, help='where the input tree and the outputs go (default: a temporary directory)')
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ensemble'))
    a = ap.parse_args()
    if a.workdir is None:
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix='xh_bench_ensemble_')
    ctx = _hip.get_context(0)
    w = synth.make_world()
    nm, S = a.months, a.members
    result = {'device': ctx.name(), 'workload': '{} cells x {} months, pm_abcd_mrtm, spin-ups 120 / 120, {} members'.format(
        w.ncell, nm, S)}
    result['statistics_kernel'] = kernel_bench(ctx, w.ncell, nm)
    if not a.kernel_only:
        # members: forcing generated on the device (the benchmark world's distributions), kept in page-locked host arrays
        d_lat = ctx.upload(w.latitude)
        dev = {k: ctx.empty((w.ncell, nm)) for k in synth.FORCING_NAMES}
        members = []
        for k in range(S):
            ctx.synth_forcing(100 + k, w.ncell, nm, d_lat, dev, nan_frac=0.001)
            host = {name: ctx.pinned((w.ncell, nm)) for name in synth.FORCING_NAMES}
            for name in synth.FORCING_NAMES:
                ctx.d2h_async(host[name], dev[name])
            ctx.sync()
            members.append(('m{:02d}'.format(k), {setting: host[name] for setting, name in SETTINGS.items()}))
        for arr in list(dev.values()) + [d_lat]:
            arr.free()
        shutil.rmtree(a.workdir, ignore_errors=True)
        os.makedirs(a.workdir)
        first = {name: members[0][1][setting] for setting, name in SETTINGS.items()}
        ini = synth.write_example(a.workdir, w, first, 1961, 1961 + nm // 12 - 1, runoff_spinup=120, routing_spinup=120,
                                  output_vars=('q', 'avgchflow'), output_format=4)
        out_dir = os.path.join(a.workdir, 'output', 'pm_abcd_mrtm_synth')
        # (a) the loop of single runs, warm (one run first)
        Xanthos(ini).execute(dict(members[0][1], OutputFolder=os.path.join(out_dir, 'warm')))
        t = time.perf_counter()
        for name, overrides in members:
            Xanthos(ini).execute(dict(overrides, OutputFolder=os.path.join(out_dir, 'single_' + name)))
        base_ms = 1e3 * (time.perf_counter() - t) / S
        result['baseline_loop_ms_per_member'] = base_ms
        # (b) the ensemble
        runs = {}
        for tag, kw in (('stats_only', dict(statistics=['mean'], member_outputs=0)), ('npy_outputs', dict(member_outputs=1))):
            for overlap in (True, False):
                run_ensemble(ini, members=members[:2], overlap=overlap, **kw)          # warm: contexts, rings
                t = time.perf_counter()
                res = run_ensemble(ini, members=members, overlap=overlap, **kw)
                ms = 1e3 * (time.perf_counter() - t) / S
                runs['{}_{}'.format(tag, 'overlapped' if overlap else 'serial')] = {
                    'ms_per_member': ms, 'ratio_to_baseline': ms / base_ms,
                    'phases_ms_per_member': {k: 1e3 * float(np.mean(res.timings[k])) for k in ('upload', 'kernels', 'post', 'write')},
                    'statistics_ms': 1e3 * res.timings['statistics']}
        result['ensemble'] = runs
        shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.out, exist_ok=True)
    name = 'bench_ensemble_kernel.json' if a.kernel_only else 'bench_ensemble.json'
    with open(os.path.join(a.out, name), 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    if not a.kernel_only:
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write(readme(result))
    print(json.dumps(result))


def readme(r):
    k = r['statistics_kernel']
    lines = ['# Ensemble run: measurements', '', 'Written by `tools/bench_ensemble.py` on {}.'.format(r['device']), '',
             'Workload: {}.'.format(r['workload']), '', '| path | ms per member | ratio to the loop of single runs |', '|---|---|---|',
             '| (a) warm loop of `Xanthos(ini).execute(args_k)`, npy outputs | {:.1f} | 1.00 |'.format(r['baseline_loop_ms_per_member'])]
    for tag, v in sorted(r['ensemble'].items()):
        lines.append('| (b) `run_ensemble`, {} | {:.1f} | {:.2f} |'.format(tag.replace('_', ' '), v['ms_per_member'], v['ratio_to_baseline']))
    lines += ['', '| phase (ms per member) | ' + ' | '.join(sorted(r['ensemble'])) + ' |', '|---|' + '---|' * len(r['ensemble'])]
    for ph in ('upload', 'kernels', 'post', 'write'):
        lines.append('| {} | '.format(ph) + ' | '.join('{:.1f}'.format(r['ensemble'][t]['phases_ms_per_member'][ph])
                                                       for t in sorted(r['ensemble'])) + ' |')
    lines += ['', '| (c) statistics kernel (mean, std, q10, q50, q90) | ms | algorithmic GB | GB/s |', '|---|---|---|---|']
    for tag in sorted(x for x in k if x.startswith('S')):
        lines.append('| `xh_ens_stats`, {} members | {:.3f} | {:.2f} | {:.0f} |'.format(
            tag[1:], k[tag]['kernel_ms'], k[tag]['algorithmic_bytes'] / 1e9, k[tag]['GBs']))
    lines.append('| `xh_memcpy_d2d` of one array (read + write) | {:.3f} | {:.2f} | {:.0f} |'.format(
        k['memcpy_d2d']['ms'], k['memcpy_d2d']['bytes'] / 1e9, k['memcpy_d2d']['GBs']))
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    main()
