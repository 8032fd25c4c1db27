"""Numpy restatement of the gauge form of the streamflow calibration objective, test infrastructure.

Built on the oracle like flowcal_np: ABCD on ALL of the basin's cells, the rows scattered into a world of zeros, the
WHOLE world routed by oracle.mrtm.route_series (routing spin-up, then every month), Avg_ChFlow read at every gauge's cell
(nothing summed), every gauge scored by oracle.calib.kge_distance on the months with a finite observation, and the
basin's energy (sum w_g ED_g) / (sum w_g) over the gauges as given (ascending (cell, gauge id)), left to right.  It routes
the world, not the union closure, so it also checks that the union closure is all that matters.
"""
import numpy as np

from oracle import calib as o_calib, mrtm as o_mrtm

import flowcal_np


def masked_kge_distance(series, obs):
    """ED of ``series`` against ``obs`` over the months whose observation is finite."""
    v = np.isfinite(obs)
    return o_calib.kge_distance(np.asarray(series)[v], np.asarray(obs)[v])


def combine(ed_g, weights):
    """(sum w_g ED_g) / (sum w_g), left to right."""
    num = den = 0.0
    for e, w in zip(ed_g, weights):
        num = num + w * e
        den = den + w
    return num / den


def world_avg(pars, cells, um_csr, pet, precip, tmin, flow_dist, velocity, area, chs_prev, ndays, nmonths, runoff_spinup,
              routing_spinup, dt=10800):
    """Avg_ChFlow [ncell, nmonths] of routing the world with the runoff of the basin with the cells ``cells``."""
    rsim = np.zeros((pet.shape[0], nmonths))
    rsim[cells] = flowcal_np.runoff(pars, pet[cells], precip[cells], None if tmin is None else tmin[cells], nmonths,
                                    runoff_spinup)
    _, avg, _ = o_mrtm.route_series(um_csr, flow_dist, velocity, area, rsim, ndays, routing_spinup, S0=chs_prev, dt=dt)
    return avg


def objective(pars, gauge_cells, weights, obs, cells, *args, **kw):
    """(ED_B, ED_g [ng], series [ng, nmonths]) of the basin with the cells ``cells`` and the gauges on ``gauge_cells``
    (in scoring order) with records ``obs`` [ng, nmonths], NaN = missing."""
    avg = world_avg(pars, cells, *args, **kw)
    ser = avg[np.asarray(gauge_cells)]
    ed_g = np.array([masked_kge_distance(s, o[:s.size]) for s, o in zip(ser, np.asarray(obs))])
    return combine(ed_g, weights), ed_g, ser
