"""Generate gaugecal.npz, the golden vectors of the gauge form of the streamflow calibration objective (set_calibrate = 1
with stream gauges inside the network, records with gaps), from the REAL reference (JGCRI/xanthos v2.4.1).

Run in the build container only (needs the reference checkout, which the GPU box does not have):

    python tests/golden/make_golden_gaugecal.py

The reference has no gauge mode (and its set_calibrate = 1 branch cannot run at all, see make_golden_flowcal.py).  The
contract of DESIGN 4.4 is pinned here with the reference's own parts, imported unmodified by file path through
make_golden_flowcal.py: ``ABCD(..., method='dist')`` on the basin's cells, the rows scattered into a world of zeros, the
month loops of Components.calculate_routing over ``streamrouting`` on the WORLD, Avg_ChFlow read at each gauge's cell
(nothing summed), ``objective_kge`` on the compressed ``series[V]``, ``obs[V]`` (V = the months with a finite
observation), and the basin's energy (sum w_g ED_g) / (sum w_g) over its gauges in ascending (cell, gauge id) order.

World: that of flowcal.npz (600 cells, 36 months, runoff spin-up 25, routing spin-up 6), not stored again.  Gauges:
  101, 102, 103  complete records on the single outlets of basins 2, 6 and 9 (basin 9 is one headwater cell)
  104, 105       basin 5 (five outlets): an interior gauge on the main stem above its largest outlet and one nested
                 upstream of it, weights 2 and 0.5, ~20 % of the months missing, the first and the last among them
  106            basin 3, on the cell below the tributary that went to basin 5 (foreign cells in the closure)
  107            basin 1 (seven outlets), one tributary gauge on a cell that may fire, gaps
  108            basin 7 (nine outlets), a headwater gauge (a closure of one cell), gaps
Cases: snow (tmin) and no snow, three parameter vectors each, as in flowcal.npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden_flowcal as fc  # noqa: E402  (loads the reference's modules by path)

NM, SPIN, RSPIN, DT = fc.NM, fc.SPIN, fc.RSPIN, fc.DT


def upstream_lists(um):
    coo = um.tocoo()
    ups = {}
    for r, c, v in zip(coo.row, coo.col, coo.data):
        if v > 0 and r != c:
            ups.setdefault(int(r), []).append(int(c))
    return ups


def closure(ups, i):
    out, todo = set(), [int(i)]
    while todo:
        j = todo.pop()
        if j not in out:
            out.add(j)
            todo.extend(ups.get(j, []))
    return sorted(out)


def choose_gauges(W):
    """(gauge_id, cell, weight) rows; every choice is the first cell in ascending order that fits."""
    um, bid, dsid = W['um'], W['basin_ids'], W['dsid']
    ups = upstream_lists(um)
    fires = W['velocity'] * DT > W['flow_dist']
    outl = {b: fc.outlets(um, np.nonzero(bid == b)[0]) for b in range(1, 10)}
    rows = []
    for gid, b in ((101, 2), (102, 6), (103, 9)):
        assert outl[b].size == 1
        rows.append((gid, int(outl[b][0]), 1.0))
    # basin 5: main stem = the chain of largest closures above its largest outlet; an interior gauge and one nested above
    stem, i = [], int(max(outl[5], key=lambda j: len(closure(ups, j))))
    while True:
        stem.append(i)
        up = [j for j in ups.get(i, []) if bid[j] == 5]
        if not up:
            break
        i = max(up, key=lambda j: (len(closure(ups, j)), -j))
    inner = [i for i in stem[1:] if len(closure(ups, i)) >= 8 and W['velocity'][i] > 0]      # (a still cell records zeros)
    assert len(inner) >= 2, stem
    lower, upper = inner[0], inner[-1]
    assert upper in closure(ups, lower) and upper != lower
    rows += [(104, lower, 2.0), (105, upper, 0.5)]
    # basin 3: the cell the lost tributary drains into
    below = int(dsid[W['trib'][0]] - 1)
    assert bid[below] == 3 and any(bid[j] == 5 for j in closure(ups, below))
    rows.append((106, below, 1.0))
    # basin 1: a tributary gauge on a firing cell, not an outlet, with something upstream
    assert outl[1].size > 1
    cand = [int(i) for i in np.nonzero((bid == 1) & fires)[0] if i not in outl[1] and len(closure(ups, i)) >= 3]
    rows.append((107, cand[0], 1.0))
    # basin 7: a headwater cell
    assert outl[7].size > 1
    head = [int(i) for i in np.nonzero(bid == 7)[0] if int(i) not in ups and i not in outl[7]]
    rows.append((108, head[0], 1.0))
    return np.array(rows, dtype=float), fires


def gaps(gid):
    """Months without an observation: about 20 % of them, the first and the last included (complete for 101-103)."""
    miss = np.zeros(NM, dtype=bool)
    if gid > 103:
        rng = np.random.default_rng(1000 + int(gid))
        miss[rng.choice(np.arange(1, NM - 1), size=5, replace=False)] = True
        miss[[0, NM - 1]] = True
    return miss


def world_avg(W, pars, b, tmin):
    """Avg_ChFlow [ncell, NM] of routing the world with the runoff of basin b (make_golden_flowcal.series before the sum)."""
    cells = np.nonzero(W['basin_ids'] == b)[0]
    n = cells.size
    he = fc.ref_abcd.ABCD(np.repeat(pars[None, :], n, axis=0), W['pet'][cells], W['precip'][cells],
                          None if tmin is None else tmin[cells], np.zeros(n), NM, SPIN, method='dist')
    he.emulate()
    rsim = np.zeros(W['pet'].shape)
    rsim[cells, :] = np.asarray(he.rsim).T
    chs_prev, flow = W['chs_prev'].copy(), np.zeros(rsim.shape[0])
    avg = np.zeros(rsim.shape)
    for nm in list(range(RSPIN)) + list(range(NM)):             # Components.calculate_routing (:273-294)
        S, favg, flow = fc.ref_mrtm.streamrouting(W['flow_dist'], chs_prev, flow, W['velocity'], rsim[:, nm], W['area'],
                                                  W['ndays'][nm], DT, W['um'])
        avg[:, nm] = favg
        chs_prev = np.copy(S)
    return avg


def main():
    W = fc.world()
    g = np.load(os.path.join(HERE, 'flowcal.npz'))
    for k in ('basin_ids', 'flow_dist', 'velocity', 'area', 'chs_prev', 'precip', 'tmin', 'pet', 'ndays'):
        assert np.array_equal(W[k], g[k]), k                    # the world of flowcal.npz, which the tests load
    assert np.array_equal(W['um'].indices, g['indices'])
    gauges, fires = choose_gauges(W)
    gid, gcell, gw = gauges[:, 0].astype(int), gauges[:, 1].astype(int), gauges[:, 2]
    gbasin = W['basin_ids'][gcell]
    assert fires[gcell[gid == 107][0]]
    order = np.lexsort((gid, gcell, gbasin))                    # basin after basin, ascending (cell, gauge id) inside
    gid, gcell, gw, gbasin = gid[order], gcell[order], gw[order], gbasin[order]
    basins = np.unique(gbasin)
    pars, truth = g['pars'], np.array([0.9, 1.2, 0.4, 0.5, 0.5])
    miss = np.stack([gaps(i) for i in gid])
    out = dict(gauge_id=gid, gauge_cell=gcell, gauge_weight=gw, gauge_basin=gbasin, basins=basins, pars=pars,
               truth=truth)
    for tag, tmin in (('snow', W['tmin']), ('nosnow', None)):
        npar = 5 if tmin is not None else 4
        obs = np.zeros((gid.size, NM))
        ser = np.zeros((gid.size, len(pars), NM))
        edg = np.zeros((gid.size, len(pars)))
        ed = np.zeros((basins.size, len(pars)))
        for bi, b in enumerate(basins):
            sel = np.nonzero(gbasin == b)[0]
            t = world_avg(W, truth[:npar], b, tmin)
            for k in sel:
                obs[k] = t[gcell[k]] * (1 + 0.1 * np.sin(np.arange(NM)))
                obs[k, miss[k]] = np.nan
                assert np.nanstd(obs[k]) > 0 and np.nanmean(obs[k]) != 0, gid[k]
            for j, p in enumerate(pars):
                avg = world_avg(W, p[:npar], b, tmin)
                num = den = 0.0
                for k in sel:
                    s = avg[gcell[k]].copy()
                    v = np.isfinite(obs[k])
                    ser[k, j] = s
                    edg[k, j] = fc.ref_cal.objective_kge(p[:npar], lambda *a: s[v], 1, None, None, None, NM, SPIN,
                                                         'm3_per_sec', None, obs[k][v], None, None)
                    num = num + gw[k] * edg[k, j]
                    den = den + gw[k]
                ed[bi, j] = num / den
        out[tag + '_obs'], out[tag + '_series'], out[tag + '_ed_gauge'], out[tag + '_ed'] = obs, ser, edg, ed
    path = os.path.join(HERE, 'gaugecal.npz')
    np.savez_compressed(path, **out)
    print('gaugecal.npz', os.path.getsize(path), 'bytes')
    for i, c, w, b in zip(gid, gcell, gw, gbasin):
        print('gauge', i, 'basin', b, 'cell', c, 'weight', w, 'closure', len(closure(upstream_lists(W['um']), c)),
              'fires', bool(fires[c]))


if __name__ == '__main__':
    main()
