"""Numpy restatement of the streamflow calibration objective (set_calibrate = 1), test infrastructure.

Built on the oracle: ABCD on the basin's cells (oracle.abcd.ABCD, as basin_runoff runs it), the rows scattered into a
world of zeros (the intent of calibrate_abcd.py:170-171), the WHOLE world routed by oracle.mrtm.route_series (routing
spin-up, then every month), Avg_ChFlow summed over the basin's outlets one after the other in ascending cell order, and
scored by oracle.calib.kge_distance.  It routes the world, not the closure, so it also checks that the closure is all
that matters.
"""
import numpy as np

from oracle import abcd as o_abcd, calib as o_calib, mrtm as o_mrtm


def outlets(um_csr, cells):
    """Cells of the basin whose outflow reaches no cell of the basin through UM (ascending)."""
    um = um_csr.tocoo()
    in_b = np.zeros(um.shape[0], dtype=bool)
    in_b[cells] = True
    e = (um.data > 0) & (um.row != um.col) & in_b[um.row]
    drains = np.zeros(um.shape[0], dtype=bool)
    drains[um.col[e]] = True
    return np.asarray(cells)[~drains[cells]]


def runoff(pars, pet_b, precip_b, tmin_b, nmonths, runoff_spinup):
    """[ncell_b, nmonths] mm/month of one parameter vector spread over the basin (calibrate_abcd.py:155-167)."""
    n = pet_b.shape[0]
    he = o_abcd.ABCD(np.repeat(np.asarray(pars, dtype=float)[None, :], n, axis=0), pet_b, precip_b, tmin_b, np.zeros(n),
                     nmonths, runoff_spinup)
    he.emulate()
    return np.asarray(he.rsim).T


def series(pars, cells, um_csr, pet, precip, tmin, flow_dist, velocity, area, chs_prev, ndays, nmonths, runoff_spinup,
           routing_spinup, dt=10800):
    """Outlet streamflow [nmonths] (m3/s) of the basin with the cells ``cells``."""
    ncell = pet.shape[0]
    rsim = np.zeros((ncell, nmonths))
    rsim[cells] = runoff(pars, pet[cells], precip[cells], None if tmin is None else tmin[cells], nmonths, runoff_spinup)
    _, avg, _ = o_mrtm.route_series(um_csr, flow_dist, velocity, area, rsim, ndays, routing_spinup, S0=chs_prev, dt=dt)
    out = np.zeros(nmonths)
    for i in outlets(um_csr, cells):
        out = out + avg[i]
    return out


def objective(pars, obs, *args, **kw):
    """ED = 1 - KGE of the outlet series against obs[:nmonths]."""
    s = series(pars, *args, **kw)
    return o_calib.kge_distance(s, np.asarray(obs)[:s.size]), s
