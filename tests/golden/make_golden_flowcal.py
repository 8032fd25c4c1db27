"""Generate flowcal.npz, the golden vectors of the streamflow calibration objective (set_calibrate = 1), from the REAL
reference (JGCRI/xanthos v2.4.1).

Run in the build container only (needs the reference checkout, which the GPU box does not have):

    python tests/golden/make_golden_flowcal.py

The reference's set_calibrate = 1 branch cannot run (calibrate_abcd.py:170-173: a flat np.put of the runoff, and the
whole Avg_ChFlow handed to np.corrcoef).  Its evident intent is pinned here with the reference's own parts,
imported unmodified by file path as make_golden.py does: ``ABCD(..., method='dist')`` as basin_runoff calls it (:166-167),
the rows scattered into a world of zeros (defect 1 fixed), the month loops of Components.calculate_routing (:273-294)
over ``streamrouting`` and UM from ``downstream`` / ``upstream`` / ``upstream_genmatrix``, the outlets' Avg_ChFlow summed
one after the other in ascending cell order, and ``objective_kge`` (:176-213) with a model function returning that series.

World: 600 cells of synth.make_world, 36 months, runoff_spinup 25, routing_spinup 6, a random initial channel storage,
one in twelve cells able to fire (velocity dt / length in (1.5, 4)).  Basin 3 loses a tributary to basin 5 (basin 3's
closure then holds foreign cells, basin 5 gains outlets that drain into basin 3), a headwater cell of basin 2 becomes a
basin of its own (id 9).  Cases: snow (tmin) and no snow, three parameter vectors each, basins 1, 2, 3, 5, 9.
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_abcd = _load('ref_abcd', 'xanthos/runoff/abcd.py')
ref_mrtm = _load('ref_mrtm', 'xanthos/routing/mrtm.py')
ref_general = _load('ref_general', 'xanthos/utils/general.py')
sys.modules['xanthos.runoff.abcd'] = ref_abcd          # calibrate_abcd.py imports ABCD from the package
sys.modules.setdefault('xanthos', type(sys)('xanthos'))
sys.modules.setdefault('xanthos.runoff', type(sys)('xanthos.runoff'))
ref_cal = _load('ref_cal', 'xanthos/calibrate/calibrate_abcd.py')

from xanthos_amd import synth  # noqa: E402

NM, SPIN, RSPIN, DT = 36, 25, 6, 10800


def world():
    w = synth.make_world(nrow=24, ncol=48, ncell=600, n_basins=8, seed=41)
    f = synth.make_forcing(w, NM)
    st = SimpleNamespace(ngridrow=w.nrow, ngridcol=w.ncol)
    dsid = ref_mrtm.downstream(w.coords, w.flow_dir, st)
    um = ref_mrtm.upstream_genmatrix(ref_mrtm.upstream(w.coords, dsid, st)).tocsr()
    basin_ids = np.asarray(w.basin_ids).copy()
    up = (um.tocoo())
    ups = {}
    for r, c, v in zip(up.row, up.col, up.data):
        if v > 0 and r != c:
            ups.setdefault(r, []).append(c)

    def subtree(i):
        out, todo = [], [i]
        while todo:
            j = todo.pop()
            out.append(j)
            todo.extend(ups.get(j, []))
        return out
    # basin 3: a tributary of 3..12 cells (not holding the outlet) goes to basin 5
    cand = [i for i in np.nonzero(basin_ids == 3)[0] if 3 <= len(subtree(i)) <= 12 and dsid[i] > 0
            and basin_ids[dsid[i] - 1] == 3]
    trib = subtree(cand[0])
    basin_ids[trib] = 5
    # a headwater cell of basin 2 becomes basin 9
    head = [i for i in np.nonzero(basin_ids == 2)[0] if i not in ups and dsid[i] > 0]
    basin_ids[head[0]] = 9
    rng = np.random.default_rng(7)
    flow_dist = np.asarray(w.flow_dist, dtype=float).copy()
    vel = np.asarray(w.velocity, dtype=float)
    fire = rng.random(w.ncell) < 1 / 12
    flow_dist[fire] = vel[fire] * DT / rng.uniform(1.5, 4.0, fire.sum())
    chs_prev = rng.uniform(0, 5e6, w.ncell)
    precip = np.nan_to_num(np.asarray(f['precip'], dtype=float))[:, :NM]
    tmin = np.asarray(f['abcd_tmin'], dtype=float)[:, :NM]
    pet = rng.uniform(20, 150, (w.ncell, NM))
    ndays = ref_general.set_month_arrays(NM, 1971, 1973)[:, 2]
    return dict(um=um, basin_ids=basin_ids, flow_dist=flow_dist, velocity=vel, area=np.asarray(w.area, dtype=float),
                chs_prev=chs_prev, precip=precip, tmin=tmin, pet=pet, ndays=ndays, dsid=dsid, trib=np.array(trib),
                head=head[0])


def outlets(um, cells):
    coo = um.tocoo()
    in_b = np.zeros(um.shape[0], dtype=bool)
    in_b[cells] = True
    drains = np.zeros(um.shape[0], dtype=bool)
    e = (coo.data > 0) & (coo.row != coo.col) & in_b[coo.row]
    drains[coo.col[e]] = True
    return cells[~drains[cells]]


def series(W, pars, b, tmin):
    cells = np.nonzero(W['basin_ids'] == b)[0]
    n = cells.size
    he = ref_abcd.ABCD(np.repeat(pars[None, :], n, axis=0), W['pet'][cells], W['precip'][cells],
                       None if tmin is None else tmin[cells], np.zeros(n), NM, SPIN, method='dist')
    he.emulate()
    rsim = np.zeros(W['pet'].shape)
    rsim[cells, :] = np.asarray(he.rsim).T                     # the rows of the basin (defect 1 of :170-171 fixed)
    chs_prev, flow = W['chs_prev'].copy(), np.zeros(rsim.shape[0])
    avg = np.zeros(rsim.shape)
    for nm in list(range(RSPIN)) + list(range(NM)):             # Components.calculate_routing (:273-294)
        S, favg, flow = ref_mrtm.streamrouting(W['flow_dist'], chs_prev, flow, W['velocity'], rsim[:, nm], W['area'],
                                               W['ndays'][nm], DT, W['um'])
        avg[:, nm] = favg
        chs_prev = np.copy(S)
    out = np.zeros(NM)
    for i in outlets(W['um'], cells):
        out = out + avg[i]
    return out


def main():
    W = world()
    basins = np.array([1, 2, 3, 5, 9])
    pars = np.array([[0.96, 0.8, 0.5, 0.4, 0.3], [0.7, 2.5, 0.2, 0.8, 0.6], [0.99, 0.3, 0.9, 0.1, 0.9]])
    truth = np.array([0.9, 1.2, 0.4, 0.5, 0.5])
    out = dict(indptr=W['um'].indptr, indices=W['um'].indices, data=W['um'].data.astype(np.int8),
               basin_ids=W['basin_ids'], flow_dist=W['flow_dist'], velocity=W['velocity'], area=W['area'],
               chs_prev=W['chs_prev'], precip=W['precip'], tmin=W['tmin'], pet=W['pet'], ndays=W['ndays'],
               nmonths=NM, runoff_spinup=SPIN, routing_spinup=RSPIN, dt=DT, basins=basins, pars=pars, trib=W['trib'],
               head=W['head'])
    for tag, tmin in (('snow', W['tmin']), ('nosnow', None)):
        npar = 5 if tmin is not None else 4
        obs = np.stack([series(W, truth[:npar], b, tmin) * (1 + 0.1 * np.sin(np.arange(NM))) for b in basins])
        ser = np.zeros((len(basins), len(pars), NM))
        ed = np.zeros((len(basins), len(pars)))
        for i, b in enumerate(basins):
            for j, p in enumerate(pars):
                s = series(W, p[:npar], b, tmin)
                ser[i, j] = s
                ed[i, j] = ref_cal.objective_kge(p[:npar], lambda *a: s, 1, None, None, None, NM, SPIN, 'm3_per_sec',
                                                 None, obs[i], None, None)
        out[tag + '_obs'], out[tag + '_series'], out[tag + '_ed'] = obs, ser, ed
    np.savez_compressed(os.path.join(HERE, 'flowcal.npz'), **out)
    print('flowcal.npz', os.path.getsize(os.path.join(HERE, 'flowcal.npz')), 'bytes')


if __name__ == '__main__':
    main()
