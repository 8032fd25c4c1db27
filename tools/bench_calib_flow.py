"""Streamflow calibration (set_calibrate = 1) at full size: the synthetic 67,420-cell world, 235 basins, 75 members
(popsize 15 x 5 parameters), 480 months, runoff spin-up 120, routing spin-up 120 months.  Times device DE generations on
the streamflow objective (csrc/xh_calib_flow.hip) and reports seconds per generation, member-cell-sub-steps per second
and the fraction of the fp64 issue rate the sub-steps reach (one wave-instruction per SIMD per 4 cycles, 256 CUs x 4
SIMDs, at the clock given; INSTR fp64 lane-instructions per member-cell-sub-step, counted from the kernel's no-fire
path: F = S tau, the gather's adds (about two entries per row), + erl, x dt, the compare, S + d, the next F, favg += F).

    python tools/bench_calib_flow.py [--members 75] [--gens 2] [--clock-ghz 2.4] [--instr 9] [--gauges] [--velocity]

--gauges times the gauge form of the objective on the same world: one gauge per basin, on the basin's outlet with the
largest upstream closure, complete records.  Each basin then routes that outlet's closure -- a subset of its outlet
closure -- and is scored by the masked KGE and the weighted combine.

--velocity times the velocity form (either form of the objective): the search has one more gene, the basins' velocity
scale inside --velocity-bounds (default 0.25 4), so SciPy's population rule gives --members 90 with snow.

--alternate PARENT_TOOL runs, in one job and twice over so that the machine's drift hits all alike, (a) PARENT_TOOL (the
bench_calib_flow.py of a built checkout of the parent commit) in its outlet form at 75 members, this build's (b) outlet and
(c) gauge form at 75 members and its velocity form at (d) 75 and (e) 90 members, each in a process of its own, --gens
generations per run, and writes the runs, and per form all generation times with mean, minimum and maximum, as one JSON
document to --out.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from xanthos_amd import _hip, synth  # noqa: E402
from xanthos_amd.calibrate.flow_tables import FlowTables, outlets_and_closure, um_arrays  # noqa: E402
from xanthos_amd.calibrate.gauge_tables import Gauges, GaugeTables  # noqa: E402
from xanthos_amd.routing import mrtm  # noqa: E402
from xanthos_amd.utils import set_month_arrays  # noqa: E402


def alternate(a):
    """The five forms one after the other, twice over; every run a child process of its own."""
    me = os.path.abspath(__file__)
    common = ['--gens', str(a.gens), '--months', str(a.months), '--spinup', str(a.spinup), '--routing-spinup',
              str(a.routing_spinup), '--clock-ghz', str(a.clock_ghz), '--instr', str(a.instr)]
    forms = [('parent_outlets', os.path.abspath(a.alternate), ['--members', '75']),
             ('outlets', me, ['--members', '75']),
             ('gauges', me, ['--members', '75', '--gauges']),
             ('velocity_75', me, ['--members', '75', '--velocity']),
             ('velocity_90', me, ['--members', '90', '--velocity'])]
    out = {name: dict(runs=[]) for name, _, _ in forms}
    for _ in range(2):
        for name, tool, extra in forms:
            env = dict(os.environ)
            env.pop('XH_LIBRARY', None)                         # every tool loads the library of its own tree
            r = subprocess.run([sys.executable, tool] + common + extra, env=env, stdout=subprocess.PIPE, text=True,
                               timeout=900, check=True)
            run = json.loads(r.stdout.strip().splitlines()[-1])
            print(name, run['generation_s'], flush=True)
            out[name]['runs'].append(run)
    for name in out:
        g = [x for run in out[name]['runs'] for x in run['generation_s']]
        out[name].update(generation_s=g, mean_s=round(float(np.mean(g)), 3), min_s=min(g), max_s=max(g),
                         member_cell_substeps_per_s=float('%.4g' % (out[name]['runs'][0]['member_cell_substeps'] / np.mean(g))))
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps({k: dict(mean_s=v['mean_s'], min_s=v['min_s'], max_s=v['max_s']) for k, v in out.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=75)
    ap.add_argument('--gens', type=int, default=2)
    ap.add_argument('--months', type=int, default=480)
    ap.add_argument('--spinup', type=int, default=120)
    ap.add_argument('--routing-spinup', type=int, default=120)
    ap.add_argument('--clock-ghz', type=float, default=2.4)
    ap.add_argument('--instr', type=float, default=9.0)
    ap.add_argument('--gauges', action='store_true', help='the gauge form: one gauge per basin on its largest-closure outlet')
    ap.add_argument('--velocity', action='store_true', help='the velocity form: the basins\' velocity scale is a gene')
    ap.add_argument('--velocity-bounds', type=float, nargs=2, default=(0.25, 4.0))
    ap.add_argument('--alternate', metavar='PARENT_TOOL', help='alternate the parent commit\'s tool and this build\'s forms')
    ap.add_argument('--out', help='--alternate: the JSON document to write')
    a = ap.parse_args()
    if a.alternate:
        return alternate(a)
    nm, spin, rspin, members = a.months, a.spinup, a.routing_spinup, a.members
    ctx = _hip.get_context(0)
    t0 = time.perf_counter()
    w = synth.make_world()
    f = {k: ctx.empty((w.ncell, nm)) for k in synth.FORCING_NAMES}
    ctx.synth_forcing(5, w.ncell, nm, ctx.upload(w.latitude), f, nan_frac=0.0)
    st = SimpleNamespace(ngridrow=w.nrow, ngridcol=w.ncol)
    um = mrtm.upstream_genmatrix(mrtm.upstream(w.coords, mrtm.downstream(w.coords, w.flow_dir, st), st))
    ndays = set_month_arrays(nm, 1971, 1971 + nm // 12 - 1)[:, 2]
    basins = list(range(1, w.n_basins + 1))
    rng = np.random.default_rng(0)
    ft = FlowTables(um, w.basin_ids, basins, w.flow_dist, w.velocity, w.area, None, ndays, nm, rspin)
    obs = rng.uniform(50, 500, (len(basins), nm))
    if a.gauges:
        ip, ix, sg = um_arrays(um)
        cells = [int(max(out, key=lambda o: outlets_and_closure(ip, ix, sg, np.array([o]))[1].size)) for out in ft.outlets]
        ft = GaugeTables(um, w.basin_ids, basins, Gauges(np.arange(len(basins)) + 1, cells, None, obs), w.flow_dist,
                         w.velocity, w.area, None, ndays, nm, rspin)
        obs = ft.obs
    # per basin: forcing rows gathered and transposed to [month, cell] ('rsds', 30..330, stands in for PET)
    pet_t, pr_t, tn_t = [], [], []
    for cells in ft.basin_cells:
        n = cells.size
        rows = ctx.upload(cells, dtype=np.int64)
        for k, lst in (('rsds', pet_t), ('precip', pr_t), ('abcd_tmin', tn_t)):
            tmp = ctx.empty((n, nm))
            ctx.gather_rows(f[k], rows, n, nm, tmp)
            t = ctx.empty((nm, n))
            ctx.transpose(tmp, n, nm, t)
            tmp.free()
            lst.append(t)
        rows.free()
    ctx.sync()
    bounds = [(1e-4, 1 - 1e-4), (1e-4, 8 - 1e-4), (1e-4, 1 - 1e-4), (1e-4, 1 - 1e-4), (1e-4, 1 - 1e-4)]
    if a.velocity:
        bounds.append(tuple(a.velocity_bounds))
    setup = time.perf_counter() - t0
    de = _hip.CalibDE(ctx, [c.size for c in ft.basin_cells], nm, spin, members, bounds, pet_t, pr_t, tn_t, None, obs,
                      seed=7, keys=basins, flow=ft, **(dict(velocity=True) if a.velocity else {}))
    t1 = time.perf_counter()
    de.init()
    t_init = time.perf_counter() - t1
    gens = []
    for _ in range(a.gens):
        ctx.timing_reset()
        t1 = time.perf_counter()
        de.step(1, tol=0.0)
        gens.append(time.perf_counter() - t1)
    ms_flow, _ = ctx.timing('calib_flow')
    ms_spin, _ = ctx.timing('calib_abcd')
    de.close()
    nt = np.floor(ndays.astype(np.int64) * 86400 / 10800).astype(np.int64)
    subs = int(nt[:rspin].sum() + nt.sum())
    cells = int(sum(c.size for c in ft.closures))
    mcs = cells * members * subs
    sec = min(gens)
    rate = mcs / sec
    peak = 256 * 4 * 64 * a.clock_ghz * 1e9 / 4             # fp64 lane-instructions per second at full issue
    res = dict(form=('gauges' if a.gauges else 'outlets') + ('+velocity' if a.velocity else ''), world_cells=int(w.ncell), basins=len(basins), closure_cells=cells, largest_closure=int(max(c.size for c in ft.closures)),
               members=members, months=nm, routing_spinup=rspin, substeps=subs, member_cell_substeps=mcs,
               setup_s=round(setup, 2), init_s=round(t_init, 3), generation_s=[round(g, 3) for g in gens],
               kernels_last_generation_ms=dict(calib_flow=round(ms_flow, 1), calib_abcd=round(ms_spin, 1)),
               member_cell_substeps_per_s=float('%.4g' % rate), instr_per_member_cell_substep=a.instr,
               clock_ghz=a.clock_ghz, fp64_issue_fraction=round(rate * a.instr / peak, 4))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
