"""Numpy restatement of the velocity forms of the streamflow calibration objective, test infrastructure.

A member's parameters are [a, b, c, d, (m), v]: the ABCD genes and, last, the basin's velocity scale v > 0.  The channel
velocity of the basin's OWN cells is multiplied by v (v * ChV, then oracle.mrtm forms tau^-1 = ChV' / L on that array as
mrtm.py:42 does); every other cell of the world -- the closure's foreign cells among them -- keeps its velocity.  The
rest is flowcal_np / gaugecal_np unchanged: the WHOLE world is routed, so this also checks that the closure is all that
matters and that foreign cells are left alone.
"""
import numpy as np

import flowcal_np
import gaugecal_np


def scaled_velocity(velocity, cells, v):
    """ChV' of the world: v * ChV on ``cells``, ChV elsewhere."""
    vel = np.array(velocity, dtype=np.float64, copy=True)
    vel[cells] = np.float64(v) * vel[cells]
    return vel


def series(pars_v, cells, um_csr, pet, precip, tmin, flow_dist, velocity, area, chs_prev, ndays, nmonths, runoff_spinup,
           routing_spinup, dt=10800):
    """Outlet streamflow [nmonths] (m3/s) of the basin with the cells ``cells`` for [a, b, c, d, (m), v]."""
    pars_v = np.asarray(pars_v, dtype=float)
    return flowcal_np.series(pars_v[:-1], cells, um_csr, pet, precip, tmin, flow_dist,
                             scaled_velocity(velocity, cells, pars_v[-1]), area, chs_prev, ndays, nmonths, runoff_spinup,
                             routing_spinup, dt=dt)


def objective(pars_v, obs, *args, **kw):
    """(ED, series) of the outlet form."""
    from oracle import calib as o_calib
    s = series(pars_v, *args, **kw)
    return o_calib.kge_distance(s, np.asarray(obs)[:s.size]), s


def gauge_objective(pars_v, gauge_cells, weights, obs, cells, um_csr, pet, precip, tmin, flow_dist, velocity, *args, **kw):
    """(ED_B, ED_g [ng], series [ng, nmonths]) of the gauge form for [a, b, c, d, (m), v]."""
    pars_v = np.asarray(pars_v, dtype=float)
    return gaugecal_np.objective(pars_v[:-1], gauge_cells, weights, obs, cells, um_csr, pet, precip, tmin, flow_dist,
                                 scaled_velocity(velocity, cells, pars_v[-1]), *args, **kw)
