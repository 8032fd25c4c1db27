"""Where the cycles of the time-skewed routing kernel go, per unit (library built with -DXH_WAVE_PROFILE, below):
ordinary groups of 16 sub-steps, groups with a month boundary, checks + month bookkeeping -- and, per class of unit, the
split of the last: checks without their waits, the waits, finalize(), the zone exit, what else lies between the runs of
groups.  The accounting reads a timer at every mark, which the buckets include: indicative, a few per cent slower than the
shipped build.  Run on the GPU box."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
os.environ['XH_FLOW_STATS'] = '1'
from xanthos_amd import _hip, synth
# make -C xanthos_amd/csrc prof (bit-exact kernel) / make exprsum EXPNAME=rprof EXPFLAGS=-DXH_WAVE_PROFILE (default kernel)
_hip.LIB_PATH = os.path.join(os.path.dirname(_hip.LIB_PATH), os.environ.get('XH_PROFILE_LIB', 'libxanthos_hip_prof.so'))
from xanthos_amd.pipeline import pipeline_from_world

months = int(sys.argv[1]) if len(sys.argv) > 1 else 240
ctx = _hip.get_context(0)
w = synth.make_world()
pipe = pipeline_from_world(ctx, w, months, 1961, 60, 0, route_flags=int(os.environ.get('XH_PROFILE_ROUTE_FLAGS', '0')))
ctx.synth_forcing(1, pipe.ncell, pipe.nmonths, ctx.upload(w.latitude), pipe.alloc_forcing(), nan_frac=0.0)
pipe.run(('pm', 'abcd'))
for rep in range(2):
    ctx.timing_reset()
    pipe.run_mrtm()
    ms, n = ctx.timing('mrtm_route')
st = pipe.plan.stats()
raw3 = st[:, 3]
shape = (raw3 & np.uint64(255)).astype(int)
zg = ((raw3 >> np.uint64(44)) & np.uint64(0x7ffff)).astype(np.float64)
# the diagnostic build packs 32-bit halves (wave_unit(), XH_WAVE_PROFILE): st[1] the run | the waits inside the checks << 32,
# st[2] housekeeping | checks with their waits << 32, st[5] zone exits | finalize() << 32
lo32 = np.uint64(0xffffffff)
raw = st
waits, total_c = (raw[:, 1] >> np.uint64(32)).astype(np.float64), (raw[:, 1] & lo32).astype(np.float64)
p_check, p_hk = (raw[:, 2] >> np.uint64(32)).astype(np.float64), (raw[:, 2] & lo32).astype(np.float64)
p_fin, p_zx = (raw[:, 5] >> np.uint64(32)).astype(np.float64), (raw[:, 5] & lo32).astype(np.float64)
# the split of check() (libraries since profiles/check_path; zeros from an older one): st[0] / st[4] carry, above their 32-bit
# cycle counts, the statement that drains the wave's memory operations with the counter loads it asked for, and the waits for a
# counter that did have to poll; st[3] bits 24-39 the checks that asked for a counter
p_drain, p_poll = (raw[:, 0] >> np.uint64(32)).astype(np.float64), (raw[:, 4] >> np.uint64(32)).astype(np.float64)
n_looks = ((raw3 >> np.uint64(24)) & np.uint64(0xffff)).astype(np.float64)
st = st.astype(np.float64)
st[:, 0] = (raw[:, 0] & lo32).astype(np.float64)
st[:, 4] = (raw[:, 4] & lo32).astype(np.float64)
st[:, 1] = total_c
st[:, 5] = p_check + p_hk + p_fin + p_zx      # "checks + months", as before the split
nsub = sum(int(d) * 8 for d in pipe.ndays)
groups = nsub / 16.0
print('route ms', ms / n, 'reassociated', pipe.plan.rsum_info())
plain, total, zone, fin = st[:, 0], st[:, 1], st[:, 4], st[:, 5]
print('units', len(st), 'boundary groups per unit: median %.0f of %.0f' % (np.median(zg), groups))
if pipe.plan.info()['last_tree_kernel'] == 4:      # k_mrtm_rsum: by streams and entry size (bit 64: 8-byte entries = single units)
    for flag, name in ((0, 'no streams'), (16, 'imports'), (32, 'exports'), (48, 'both')):
        for pl in (0, 64):
            sel = ((shape & 48) == flag) & ((shape & 64) == pl)
            if not sel.any():
                continue
            og = groups - zg[sel]
            print('%-10s %-6s n=%4d | cycles per sub-step: ordinary groups %.0f (p90 %.0f), boundary groups %.0f (p90 %.0f) | per sub-step of the run: '
                  'ordinary %.0f boundary %.0f checks+months %.0f total %.0f (max %.0f)' % (
                      name, 'single' if pl else 'pair', sel.sum(), np.median(plain[sel] / og / 16), np.percentile(plain[sel] / og / 16, 90),
                      np.median(zone[sel] / zg[sel] / 16), np.percentile(zone[sel] / zg[sel] / 16, 90),
                      np.median(plain[sel] / nsub), np.median(zone[sel] / nsub), np.median(fin[sel] / nsub), np.median(total[sel] / nsub),
                      (total[sel] / nsub).max()))
    # the split of "checks + months", per class of unit: cycles per sub-step of the run and, for the three parts that run once a
    # month, cycles per month
    nmon = float(len(pipe.ndays))
    print('split of checks+months (median per class): checks without waits | waits | finalize | zone exit | housekeeping + transitions, '
          'cycles per sub-step of the run; in brackets cycles per month')
    classes = [(name, pl, ((shape & 48) == flag) & ((shape & 64) == pl)) for flag, name in ((0, 'no streams'), (16, 'imports'), (32, 'exports'), (48, 'both'))
               for pl in (0, 64)]
    slow = np.argsort(-(total - waits))[:40]
    pace = np.zeros(len(shape), dtype=bool)
    pace[slow] = True
    classes.append(('slowest 40', 64, pace))
    fold = (raw3 >> np.uint64(63)) != 0      # the unit carries folded leaves
    classes.append(('no str fold', 64, fold & ((shape & 48) == 0)))
    classes.append(('export fold', 64, fold & ((shape & 48) == 32)))
    for name, pl, sel in classes:
        if not sel.any():
            continue
        med = lambda x: np.median(x[sel])
        print('%-11s %-6s n=%4d | %5.1f | %5.1f | %5.1f (%4.0f) | %5.1f (%4.0f) | %5.1f (%4.0f) | outside waits %.0f' % (
            name, 'single' if pl else 'pair', sel.sum(), med((p_check - waits) / nsub), med(waits / nsub), med(p_fin / nsub), med(p_fin / nmon),
            med(p_zx / nsub), med(p_zx / nmon), med(p_hk / nsub), med(p_hk / nmon), med((total - waits) / nsub)))
    # check() in three parts, cycles per sub-step of the run: (a + b) the drain up to vmcnt(0) with the counter loads the build /
    # the switch XH_FLOW_LOOK_ALWAYS asked for -- run both ways, the difference is what the loads add; (c) polls that had to poll;
    # the rest of check() (publication, guards, the timers of this build); and how many of the checks asked for a counter
    n_checks = float((nsub + 255) // 256)
    top = np.zeros(len(shape), dtype=bool)
    top[np.argsort(-(total - waits))[:10]] = True
    pairx = ((shape & 64) == 0) & ((shape & 32) != 0) if pipe.plan.rsum_info()['pair_cells'] >= 0 else np.zeros(len(shape), dtype=bool)
    print('split of check() (median per class), XH_FLOW_LOOK_ALWAYS=%s: drain + counter loads | polls that polled | rest of check() | '
          'cycles per check in the drain | checks that asked for a counter, of %d' % (os.environ.get('XH_FLOW_LOOK_ALWAYS', '0'), n_checks))
    for name, pl, sel in classes + [('top 10', 64, top), ('pair+outlet', 0, pairx)]:
        if not sel.any():
            continue
        med = lambda x: np.median(x[sel])
        print('%-11s %-6s n=%4d | %5.2f | %5.2f | %5.2f | %6.0f | %4.0f' % (
            name, 'single' if pl else 'pair', sel.sum(), med(p_drain / nsub), med(p_poll / nsub), med((p_check - p_drain - p_poll) / nsub),
            med(p_drain / n_checks), med(n_looks)))
    pu = np.nonzero((shape & 64) == 0)[0] if pipe.plan.rsum_info()['pair_cells'] >= 0 else []
    for u in pu:
        og = groups - zg[u]
        print('pair unit %4d: ordinary groups %.0f, boundary groups %.0f (%d of %d groups) | of the run: ordinary %.0f boundary %.0f checks+months %.0f total %.0f' % (
            u, plain[u] / og / 16, zone[u] / zg[u] / 16, zg[u], groups, plain[u] / nsub, zone[u] / nsub, fin[u] / nsub, total[u] / nsub))
    sys.exit(0)
for flag, name in ((0, 'isolated'), (16, 'imports'), (32, 'exports'), (48, 'both')):
    for pl in (0, 64):
        for reads in range(1, 10):
            sel = ((shape & 15) == reads + 1) & ((shape & 48) == flag) & ((shape & 64) == pl)
            if sel.sum() < 3:
                continue
            og = groups - zg[sel]
            print('%-8s %-5s %d reads n=%4d | cycles per sub-step: ordinary groups %.0f, boundary groups %.0f | per sub-step of the run: '
                  'ordinary %.0f boundary %.0f checks+months %.0f total %.0f' % (
                      name, 'plain' if pl else 'pair', reads, sel.sum(), np.median(plain[sel] / og / 16), np.median(zone[sel] / zg[sel] / 16),
                      np.median(plain[sel] / nsub), np.median(zone[sel] / nsub), np.median(fin[sel] / nsub), np.median(total[sel] / nsub)))
