"""Hargreaves-Samani monthly PET -- drop-in for xanthos/pet/hargreaves_samani.py on MI355X.

Same plugin entry point as the reference (components.py:193-195):

    execute(config, data, out_file=None) -> [ncell, nmonths]

which the reference evaluates as one scalar ``pet()`` call per cell and month (hargreaves_samani.py:95-119); here the whole
series is one launch of k_hs_pet (csrc/xh_pet_ext.hip).  ``hs_device`` / ``run_hs`` are the device and host-array entries.
The reference's formula is kept as written: t < 0 gives 0, NaN inputs give NaN, the arccos outside [-1, 1] gives 0 (polar
day as well as polar night), and ra has no sin(phi) sin(delta) term (:60).
"""
import calendar

import numpy as np

from .. import _hip


def days_per_month(start_year, end_year):
    """Days of each month of the run, leap years by the Gregorian rule (hargreaves_samani.py:18-28)."""
    return [calendar.monthrange(yr, mth)[1] for yr in range(start_year, end_year + 1) for mth in range(1, 13)]


def hs_device(ctx, ncell, nmonths, d_tas, d_tmax, d_tmin, d_lat_deg, ndays, d_pet=None):
    """Device-resident variant: d_* are DeviceArrays in HBM (d_lat_deg: latitude in degrees, coords[:, 2]); ndays the
    host list of days per month.  Returns the PET DeviceArray [ncell, nmonths]."""
    if d_pet is None:
        d_pet = ctx.empty((ncell, nmonths))
    ctx.hs_pet(ncell, nmonths, d_tas, d_tmax, d_tmin, d_lat_deg, ndays, d_pet)
    return d_pet


def run_hs(tas, tmax, tmin, lat_deg, start_year, end_year, device=0):
    """PET [ncell, nmonths] of the whole series from host arrays (NaN kept, as the loader keeps it)."""
    ctx = _hip.get_context(device)
    tas = np.asarray(tas, dtype=np.float64)
    ncell, nmonths = tas.shape
    nd = days_per_month(start_year, end_year)
    if nmonths != len(nd):
        raise ValueError('hs_tas has {} months, {}..{} has {}'.format(nmonths, start_year, end_year, len(nd)))
    bufs = [ctx.upload(tas), ctx.upload(np.asarray(tmax, dtype=np.float64)), ctx.upload(np.asarray(tmin, dtype=np.float64)),
            ctx.upload(np.asarray(lat_deg, dtype=np.float64).reshape(-1))]
    d_pet = hs_device(ctx, ncell, nmonths, *bufs, nd)
    out = d_pet.download()
    for b in bufs + [d_pet]:
        b.free()
    return out


def execute(config, data, out_file=None):
    """PET in mm/month [ncell, nmonths] (hargreaves_samani.py:95-124): data.hs_tas / hs_tmax / hs_tmin and the latitude
    in degrees of data.coords[:, 2]; saved to out_file (.npy) if given."""
    pet = run_hs(data.hs_tas, data.hs_tmax, data.hs_tmin, np.asarray(data.coords)[:, 2], config.StartYear, config.EndYear,
                 device=getattr(config, 'device', 0))
    if out_file is not None:
        np.save(out_file, pet)
    return pet
