"""The scoring at stream gauges in HBM (``xh_gauge_skill``) against the path it replaces, at full size (67,420 cells x 600
months, ``synth.make_world()`` defaults).

    python tools/bench_gauge_skill.py [--months 600] [--members 8] [--workdir DIR]      # writes the JSON and README
    python tools/bench_gauge_skill.py --kernel-only                                      # (a) and (b) alone

(a) ``xh_gauge_skill`` on one Avg_ChFlow-sized array for 235 and for 10,000 gauges (records with 20 % gaps), with the
    hydrographs written: time of the library's ``gauge_skill`` timer, and the bytes it has to move -- per gauge two reads of
    its flow row and of its record (the second from cache at best) and one write of the row: counted once each, 3 x nmonths x
    8 B per gauge;
(b) the path it replaces, in the same process: the array downloaded, the gauge rows picked and the eight columns formed in
    numpy (vectorised over the gauges), each step timed on the host clock;
(c) a resident statistics-only ensemble (``member_outputs = 0``, the mean, ``abcd_pars`` members, pm_abcd_mrtm, spin-ups 120 /
    120) without gauges and with 235 gauges: wall milliseconds per member of the whole call, and the host time of reading and
    checking the gauge files, which that call pays once.
Results: profiles/gauge_skill/bench_gauge_skill.json and the tables in profiles/gauge_skill/README.md."""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from xanthos_amd import _hip, run_ensemble, synth      # noqa: E402

GAUGE_COUNTS = (235, 10000)


def gauge_case(ncell, nmonths, ngauge, seed=9):
    rng = np.random.default_rng(seed + ngauge)
    cells = np.sort(rng.choice(ncell, size=ngauge, replace=ngauge > ncell)).astype(np.int32)
    obs = rng.uniform(5.0, 500.0, size=(ngauge, nmonths))
    obs[rng.random(obs.shape) < 0.2] = np.nan
    return cells, obs


def numpy_metrics(rows, obs):
    """The eight columns of every gauge, vectorised (NaN-aware sums over the months with an observation)."""
    v = np.isfinite(obs)
    n = v.sum(1).astype(np.float64)
    s, o = np.where(v, rows, 0.0), np.where(v, obs, 0.0)
    ms, mo = s.sum(1) / n, o.sum(1) / n
    ds, do = np.where(v, rows - ms[:, None], 0.0), np.where(v, obs - mo[:, None], 0.0)
    vss, voo, vso = (ds * ds).sum(1), (do * do).sum(1), (ds * do).sum(1)
    with np.errstate(all='ignore'):
        r = np.clip(vso / np.sqrt(vss) / np.sqrt(voo), -1.0, 1.0)
        alpha, beta = np.sqrt(vss / n) / np.sqrt(voo / n), ms / mo
        d = np.where(v, rows - obs, 0.0)
        sse = (d * d).sum(1)
        return np.stack([n, np.sqrt((r - 1) ** 2 + (alpha - 1) ** 2 + (beta - 1) ** 2), r, alpha, beta, 1.0 - sse / voo,
                         100.0 * d.sum(1) / o.sum(1), np.sqrt(sse / n)], 1)


def kernel_bench(ctx, w, nmonths, reps=20):
    ncell = w.ncell
    d_lat = ctx.upload(w.latitude)
    flow = ctx.empty((ncell, nmonths))
    ctx.synth_forcing(1, ncell, nmonths, d_lat, {'tas': flow})      # a monthly array of the benchmark world (a few NaNs included)
    out = {}
    t = time.perf_counter()
    host = flow.download()
    download_ms = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    host = flow.download(host)                                       # (the second time: pages touched, the steady figure)
    download_ms = min(download_ms, 1e3 * (time.perf_counter() - t))
    for ng in GAUGE_COUNTS:
        cells, obs = gauge_case(ncell, nmonths, ng)
        d = [ctx.upload(cells, dtype=np.int32), ctx.upload(obs), ctx.empty((ng, nmonths)), ctx.empty((ng, 8))]
        ctx.gauge_skill(ncell, nmonths, ng, d[0], flow, d[1], d[3], series=d[2])      # warm
        ctx.sync()
        ctx.timing_reset()
        for _ in range(reps):
            ctx.gauge_skill(ncell, nmonths, ng, d[0], flow, d[1], d[3], series=d[2])
        ctx.sync()
        ms, launches = ctx.timing('gauge_skill')
        got = d[3].download()
        nbytes = 3 * ng * nmonths * 8
        t = time.perf_counter()
        rows = host[cells]
        pick_ms = 1e3 * (time.perf_counter() - t)
        t = time.perf_counter()
        ref = numpy_metrics(rows, obs)
        numpy_ms = 1e3 * (time.perf_counter() - t)
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.all(np.abs(got[ok] - ref[ok]) <= 1e-9 * np.abs(ref[ok]) + 1e-9)
        out[str(ng)] = {'kernel_ms': ms / launches, 'bytes': nbytes, 'GBs': nbytes / (ms / launches) / 1e6,
                        'host_path_ms': {'download': download_ms, 'pick_rows': pick_ms, 'numpy_metrics': numpy_ms,
                                         'total': download_ms + pick_ms + numpy_ms}}
        for a in d:
            a.free()
    out['download_bytes'] = ncell * nmonths * 8
    for a in (flow, d_lat):
        a.free()
    return out


def ensemble_bench(ctx, w, nm, S, workdir):
    from bench_param_ensemble import parameter_tables
    d_lat = ctx.upload(w.latitude)
    dev = {k: ctx.empty((w.ncell, nm)) for k in synth.FORCING_NAMES}
    ctx.synth_forcing(100, w.ncell, nm, d_lat, dev, nan_frac=0.001)
    forcing = {name: dev[name].download() for name in synth.FORCING_NAMES}
    for arr in list(dev.values()) + [d_lat]:
        arr.free()
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    ini = synth.write_example(workdir, w, forcing, 1961, 1961 + nm // 12 - 1, runoff_spinup=120, routing_spinup=120,
                              output_vars=('q', 'avgchflow'), output_format=4)
    del forcing
    members = [('p{:02d}'.format(k), {'abcd_pars': t}) for k, t in enumerate(parameter_tables(w.abcd_pars, S))]
    cells, obs = gauge_case(w.ncell, nm, GAUGE_COUNTS[0])
    ids = 1000 + np.arange(cells.size)
    gauges, records = os.path.join(workdir, 'gauges.csv'), os.path.join(workdir, 'gauge_obs.csv')
    np.savetxt(gauges, np.stack([ids, cells + 1], 1), delimiter=',', fmt='%d')
    np.savetxt(records, np.array([[i, 0.0, 0.0, v] for i, row in zip(ids, obs) for v in row]), delimiter=',', fmt='%.17g')
    from xanthos_amd import ConfigReader
    from xanthos_amd.evaluate import load_gauge_set
    t = time.perf_counter()
    load_gauge_set(ConfigReader(ini), gauges, records)               # what ensemble.validate does once per call, on the host
    load_ms = 1e3 * (time.perf_counter() - t)
    runs = {}
    for tag, kw in (('without_gauges', {}), ('with_235_gauges', dict(gauges=gauges, gauge_observed=records))):
        run_ensemble(ini, members=members[:2], statistics=['mean'], member_outputs=0, **kw)      # warm: contexts, the plan
        t = time.perf_counter()
        res = run_ensemble(ini, members=members, statistics=['mean'], member_outputs=0, **kw)
        ms = 1e3 * (time.perf_counter() - t) / S
        assert all(not u for u in res.forcing_upload[1:]) and (res.gauge_kge is not None) == bool(kw)
        runs[tag] = {'ms_per_member': ms, 'statistics_ms': 1e3 * res.timings['statistics'],
                     'phases_ms_per_member': {k: 1e3 * float(np.mean(res.timings[k][1:])) for k in ('kernels', 'post', 'write')}}
    shutil.rmtree(workdir, ignore_errors=True)
    runs['with_235_gauges']['gauge_files_load_ms_once'] = load_ms
    return runs


def readme(r):
    k = r['kernel']
    lines = ['# Skill at stream gauges: measurements', '', 'Written by `tools/bench_gauge_skill.py` on {}.'.format(r['device']), '',
             'Workload: {}.  Command: `python tools/bench_gauge_skill.py{}`.'.format(r['workload'], r['arguments']), '',
             '| (a) `xh_gauge_skill`, hydrographs written | ms | MB moved (3 x nmonths x 8 B per gauge) | GB/s |', '|---|---|---|---|']
    for ng in GAUGE_COUNTS:
        v = k[str(ng)]
        lines.append('| {} gauges | {:.4f} | {:.2f} | {:.0f} |'.format(ng, v['kernel_ms'], v['bytes'] / 1e6, v['GBs']))
    lines += ['', '| (b) the path it replaces (host clock, ms) | download of Avg_ChFlow ({:.0f} MB) | rows picked | metrics in numpy | total |'
              .format(k['download_bytes'] / 1e6), '|---|---|---|---|---|']
    for ng in GAUGE_COUNTS:
        h = k[str(ng)]['host_path_ms']
        lines.append('| {} gauges | {:.1f} | {:.2f} | {:.2f} | {:.1f} |'.format(ng, h['download'], h['pick_rows'], h['numpy_metrics'],
                                                                       h['total']))
    if 'ensemble' in r:
        lines += ['', '| (c) resident ensemble, member_outputs = 0, the mean | ms per member (wall, whole call) | kernels | post | write | '
                  'statistics, once |', '|---|---|---|---|---|---|']
        for tag, v in r['ensemble'].items():
            p = v['phases_ms_per_member']
            lines.append('| {} | {:.1f} | {:.1f} | {:.1f} | {:.1f} | {:.1f} |'.format(tag.replace('_', ' '), v['ms_per_member'], p['kernels'],
                                                                              p['post'], p['write'], v['statistics_ms']))
        lines += ['', 'The whole-call figure with gauges includes reading and checking the two gauge files on the host, once per call: '
                  '{:.1f} ms here ({} gauges x {} rows of text), i.e. {:.1f} ms per member of this run.'.format(
                      r['ensemble']['with_235_gauges']['gauge_files_load_ms_once'], GAUGE_COUNTS[0], r['months'],
                      r['ensemble']['with_235_gauges']['gauge_files_load_ms_once'] / r['members'])]
    else:
        lines += ['', '(c) the resident ensemble with and without gauges: not measured in this run.']
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=8)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--workdir', default=None, help='where the input tree and the outputs go (default: a temporary directory)')
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gauge_skill'))
    a = ap.parse_args()
    if a.workdir is None:
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix='xh_bench_gauge_skill_')
    ctx = _hip.get_context(0)
    w = synth.make_world()
    result = {'device': ctx.name(), 'months': a.months, 'members': a.members, 'arguments': (' --kernel-only' if a.kernel_only else '') + (' --months {}'.format(a.months) if a.months != 600 else '') +
              (' --members {}'.format(a.members) if a.members != 8 else ''),
              'workload': '{} cells x {} months'.format(w.ncell, a.months)}
    result['kernel'] = kernel_bench(ctx, w, a.months)
    if not a.kernel_only:
        result['workload'] += '; (c) pm_abcd_mrtm, spin-ups 120 / 120, {} parameter tables'.format(a.members)
        result['ensemble'] = ensemble_bench(ctx, w, a.months, a.members, a.workdir)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_gauge_skill.json'), 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    with open(os.path.join(a.out, 'README.md'), 'w') as fh:
        fh.write(readme(result))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
