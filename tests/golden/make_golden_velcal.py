"""Generate velcal.npz, the golden vectors of the velocity forms of the streamflow calibration objective (one more
calibration parameter per basin, the velocity scale v), from the REAL reference (JGCRI/xanthos v2.4.1).

Run in the build container only (needs the reference checkout, which the GPU box does not have):

    python tests/golden/make_golden_velcal.py

The contract of DESIGN 4.4 is pinned with the reference's own parts, imported unmodified by file path through
make_golden_flowcal.py: ``ABCD(..., method='dist')`` on the basin's cells, the rows scattered into a world of zeros, the
month loops of Components.calculate_routing over ``streamrouting`` on the WORLD, the outlets' Avg_ChFlow summed in
ascending cell order (outlet form) or Avg_ChFlow read at each gauge's cell (gauge form), and ``objective_kge``.  The ONLY
change: the entries of ChV that belong to the basin are multiplied by v before ``streamrouting`` sees the array.

Worlds: those of flowcal.npz and gaugecal.npz, loaded, not stored again.  Stored: the scales, the observations, the
series and the EDs -- and the three arrays of the "pin" world (below) that differ from flowcal's.
Cases: snow and no snow, the first two parameter vectors of flowcal.npz, basins 1, 2, 3, 5, 9, scales 1, 0.5, 2, 3.5, the
outlet form and the gauge form (the gauges of gaugecal.npz in those basins) from the same routing of the world.

The generator checks three things itself and aborts otherwise:
  1. the v = 1.0 series are those of flowcal.npz / gaugecal.npz bit for bit;
  2. the pin world tells "the basin's cells are scaled" from "the whole closure is scaled".  The flowcal world does not:
     its foreign tributary (the cells basin 3 lost to basin 5) has emptied to zero after six spin-up months.  The pin
     world routes one spin-up month only and makes those cells long, slow and full, so they still drain into basin 3 in
     the scored months; the two readings must differ by more than 1e-6 relative in some month;
  3. the tolerance of the tests (1e-9 relative) is safe on these inputs: cell areas perturbed by 1e-10 relative change
     no series value by more than 1e-10 relative, for every basin and scale of the golden.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden_flowcal as fc  # noqa: E402  (loads the reference's modules by path)

NM, SPIN, RSPIN, DT = fc.NM, fc.SPIN, fc.RSPIN, fc.DT
BASINS = np.array([1, 2, 3, 5, 9])
SCALES = np.array([1.0, 0.5, 2.0, 3.5])
PIN_BASIN, PIN_RSPIN, PIN_SCALES = 3, 1, np.array([0.5, 2.0])


def world_avg(W, pars, b, tmin, v, rspin=RSPIN, whole=False):
    """Avg_ChFlow [ncell, NM] of routing the world with the runoff of basin b and ChV scaled by v on the basin's cells
    (whole: on every cell, the reading the contract rejects)."""
    cells = np.nonzero(W['basin_ids'] == b)[0]
    n = cells.size
    he = fc.ref_abcd.ABCD(np.repeat(pars[None, :], n, axis=0), W['pet'][cells], W['precip'][cells],
                          None if tmin is None else tmin[cells], np.zeros(n), NM, SPIN, method='dist')
    he.emulate()
    rsim = np.zeros(W['pet'].shape)
    rsim[cells, :] = np.asarray(he.rsim).T
    chv = W['velocity'].copy()
    if whole:
        chv = v * chv
    else:
        chv[cells] = v * chv[cells]                             # the only change to the reference's run
    chs_prev, flow = W['chs_prev'].copy(), np.zeros(rsim.shape[0])
    avg = np.zeros(rsim.shape)
    for nm in list(range(rspin)) + list(range(NM)):             # Components.calculate_routing (:273-294)
        S, favg, flow = fc.ref_mrtm.streamrouting(W['flow_dist'], chs_prev, flow, chv, rsim[:, nm], W['area'],
                                                  W['ndays'][nm], DT, W['um'])
        avg[:, nm] = favg
        chs_prev = np.copy(S)
    return avg


def outlet_sum(W, b, avg):
    out = np.zeros(NM)
    for i in fc.outlets(W['um'], np.nonzero(W['basin_ids'] == b)[0]):
        out = out + avg[i]
    return out


def kge(pars, s, obs):
    return fc.ref_cal.objective_kge(pars, lambda *a: s, 1, None, None, None, NM, SPIN, 'm3_per_sec', None, obs, None, None)


def main():
    W = fc.world()
    g = np.load(os.path.join(HERE, 'flowcal.npz'))
    gg = np.load(os.path.join(HERE, 'gaugecal.npz'))
    for k in ('basin_ids', 'flow_dist', 'velocity', 'area', 'chs_prev', 'precip', 'tmin', 'pet', 'ndays'):
        assert np.array_equal(W[k], g[k]), k                    # the world of flowcal.npz, which the tests load
    assert np.array_equal(W['um'].indices, g['indices'])
    assert np.array_equal(BASINS, g['basins'])
    pars = g['pars'][:2]
    gsel = np.nonzero(np.isin(gg['gauge_basin'], BASINS))[0]    # the gauges of gaugecal.npz in these basins, its order
    gcell, gw, gbasin = gg['gauge_cell'][gsel], gg['gauge_weight'][gsel], gg['gauge_basin'][gsel]
    out = dict(basins=BASINS, scales=SCALES, pars=pars, gauge_sel=gsel)

    # the pin world: the tributary basin 3 lost to basin 5 is long, slow and full, and one spin-up month leaves it so
    P = dict(W)
    trib = W['trib']
    P['flow_dist'], P['velocity'], P['chs_prev'] = W['flow_dist'].copy(), W['velocity'].copy(), W['chs_prev'].copy()
    P['flow_dist'][trib] = 2.0e6
    P['velocity'][trib] = 0.3
    P['chs_prev'][trib] = 5.0e9
    out.update(pin_basin=PIN_BASIN, pin_routing_spinup=PIN_RSPIN, pin_scales=PIN_SCALES, pin_flow_dist=P['flow_dist'],
               pin_velocity=P['velocity'], pin_chs_prev=P['chs_prev'])
    k106 = int(np.nonzero(gg['gauge_id'] == 106)[0][0])          # basin 3's gauge, below that tributary

    rng = np.random.default_rng(11)
    A = dict(W)
    A['area'] = W['area'] * (1.0 + 1e-10 * rng.uniform(-1, 1, W['area'].size))
    worst = 0.0

    for tag, tmin in (('snow', W['tmin']), ('nosnow', None)):
        npar = 5 if tmin is not None else 4
        obs, gobs = g[tag + '_obs'], gg[tag + '_obs'][gsel]
        ser = np.zeros((BASINS.size, len(pars), SCALES.size, NM))
        ed = np.zeros(ser.shape[:3])
        gser = np.zeros((gsel.size, len(pars), SCALES.size, NM))
        ged = np.zeros(gser.shape[:3])
        gedb = np.zeros(ser.shape[:3])
        for i, b in enumerate(BASINS):
            sel = np.nonzero(gbasin == b)[0]
            for j, p in enumerate(pars):
                for s, v in enumerate(SCALES):
                    avg = world_avg(W, p[:npar], b, tmin, v)
                    ser[i, j, s] = outlet_sum(W, b, avg)
                    ed[i, j, s] = kge(p[:npar], ser[i, j, s], obs[i])
                    num = den = 0.0
                    for k in sel:
                        gs = avg[gcell[k]].copy()
                        m = np.isfinite(gobs[k])
                        gser[k, j, s] = gs
                        ged[k, j, s] = kge(p[:npar], gs[m], gobs[k][m])
                        num = num + gw[k] * ged[k, j, s]
                        den = den + gw[k]
                    gedb[i, j, s] = num / den
                    if j == 0:                                  # condition 3: no amplification of a 1e-10 perturbation
                        sa = outlet_sum(A, b, world_avg(A, p[:npar], b, tmin, v))
                        nz = ser[i, j, s] != 0
                        assert np.array_equal(sa[~nz], ser[i, j, s][~nz])
                        rel = float(np.max(np.abs(sa[nz] - ser[i, j, s][nz]) / np.abs(ser[i, j, s][nz])))
                        worst = max(worst, rel)
                        assert rel <= 1e-10, ('area perturbation amplified', tag, b, v, rel)
        # condition 1: v = 1.0 is the existing contract, bit for bit
        assert SCALES[0] == 1.0
        assert np.array_equal(ser[:, :, 0], g[tag + '_series'][:, :2]), tag
        assert np.array_equal(ed[:, :, 0], g[tag + '_ed'][:, :2]), tag
        assert np.array_equal(gser[:, :, 0], gg[tag + '_series'][gsel][:, :2]), tag
        assert np.array_equal(ged[:, :, 0], gg[tag + '_ed_gauge'][gsel][:, :2]), tag
        bsel = np.nonzero(np.isin(gg['basins'], BASINS))[0]
        assert np.array_equal(gedb[:, :, 0], gg[tag + '_ed'][bsel][:, :2]), tag
        out[tag + '_obs'], out[tag + '_series'], out[tag + '_ed'] = obs, ser, ed
        out[tag + '_gauge_obs'], out[tag + '_gauge_series'] = gobs, gser
        out[tag + '_gauge_ed_gauge'], out[tag + '_gauge_ed'] = ged, gedb

        # condition 2: the pin world, basin 3, outlet form and gauge 106
        i3 = int(np.nonzero(BASINS == PIN_BASIN)[0][0])
        pser = np.zeros((len(pars), PIN_SCALES.size, NM))
        ped = np.zeros(pser.shape[:2])
        pgser, pged = np.zeros_like(pser), np.zeros_like(ped)
        gap = 0.0
        m106 = np.isfinite(gg[tag + '_obs'][k106])
        for j, p in enumerate(pars):
            for s, v in enumerate(PIN_SCALES):
                avg = world_avg(P, p[:npar], PIN_BASIN, tmin, v, rspin=PIN_RSPIN)
                pser[j, s] = outlet_sum(P, PIN_BASIN, avg)
                ped[j, s] = kge(p[:npar], pser[j, s], obs[i3])
                pgser[j, s] = avg[gg['gauge_cell'][k106]]
                pged[j, s] = kge(p[:npar], pgser[j, s][m106], gg[tag + '_obs'][k106][m106])
                if j == 0:
                    other = outlet_sum(P, PIN_BASIN, world_avg(P, p[:npar], PIN_BASIN, tmin, v, rspin=PIN_RSPIN, whole=True))
                    gap = max(gap, float(np.max(np.abs(other - pser[j, s]) / np.abs(pser[j, s]))))
        assert gap > 1e-6, ('the pin world does not tell the basin\'s cells from the whole closure', tag, gap)
        print(tag, 'pin: basin cells only vs whole closure differ by', gap, 'relative')
        out[tag + '_pin_series'], out[tag + '_pin_ed'] = pser, ped
        out[tag + '_pin_gauge_series'], out[tag + '_pin_gauge_ed'] = pgser, pged
    out['pin_gauge_index'] = k106
    print('area perturbation 1e-10 -> at most', worst, 'relative')
    path = os.path.join(HERE, 'velcal.npz')
    np.savez_compressed(path, **out)
    print('velcal.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
