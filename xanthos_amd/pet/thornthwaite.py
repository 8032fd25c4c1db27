"""Thornthwaite monthly PET -- drop-in for xanthos/pet/thornthwaite.py on MI355X.

Same entry points as the reference (components.py:204-206, thornthwaite.py:18-130):

    execute(tas, lat_radians, start_yr, end_yr) -> [ncell, nmonths]
    calc_daylight_hours(mth_days, lat_radians)  -> [ncell, 12]

computed by k_trn_daylight and k_trn_pet (csrc/xh_pet_ext.hip); ``thornthwaite_device`` is the device entry.  NaN and
negative temperatures count as 0; unlike the reference, ``execute`` does not zero them in the caller's ``tas`` in place.

Daylight order: the reference spreads the 12 monthly daylight means with ``np.repeat(L, nyears, axis=1)`` (:113), so
in a common year global month m gets the daylight of month-of-year m // nyears, while leap years get the leap table in
month order (:116-122).  ``daylight='reference'`` (the default) reproduces that; ``'monthly'`` gives every month its own
month's daylight.
"""
import numpy as np

from .. import _hip

MONTHDAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
LEAP_MONTHDAYS = (31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
DAYLIGHT_MODES = {'reference': _hip.XH_DAYLIGHT_REFERENCE, 'monthly': _hip.XH_DAYLIGHT_MONTHLY}


def daylight_mode(name):
    try:
        return DAYLIGHT_MODES[name]
    except KeyError:
        raise ValueError("daylight must be one of {}, not '{}'".format(tuple(DAYLIGHT_MODES), name))


def thornthwaite_device(ctx, ncell, nmonths, start_year, d_tas, d_lat, daylight='reference', d_pet=None,
                        d_daylight=None):
    """Device-resident variant: d_tas [ncell, nmonths] (whole years from start_year) and d_lat (radians) DeviceArrays in
    HBM.  Returns the PET DeviceArray; d_daylight, if given, receives the [ncell, 24] table (common year, leap year)."""
    if d_pet is None:
        d_pet = ctx.empty((ncell, nmonths))
    ctx.thornthwaite_pet(ncell, nmonths, start_year, daylight_mode(daylight), d_tas, d_lat, d_pet, d_daylight)
    return d_pet


def calc_daylight_hours(mth_days, lat_radians, device=0):
    """Mean daylight hours of each month at each latitude (thornthwaite.py:18-48) for the 12 months of a common or of
    a leap year (the two calendars the reference calls it with)."""
    mth_days = tuple(int(d) for d in mth_days)
    if mth_days not in (MONTHDAYS, LEAP_MONTHDAYS):
        raise ValueError('mth_days must be the 12 months of a common or of a leap year')
    ctx = _hip.get_context(device)
    lat = np.asarray(lat_radians, dtype=np.float64).reshape(-1)
    d_lat, d_dl = ctx.upload(lat), ctx.empty((lat.size, 24))
    ctx.thornthwaite_pet(lat.size, 0, 1970, _hip.XH_DAYLIGHT_REFERENCE, None, d_lat, None, d_dl)
    dl = d_dl.download()
    for b in (d_lat, d_dl):
        b.free()
    return np.ascontiguousarray(dl[:, 12:] if mth_days == LEAP_MONTHDAYS else dl[:, :12])


def execute(tas, lat_radians, start_yr, end_yr, daylight='reference', device=0):
    """PET in mm/month [ncell, nmonths] from mean monthly temperature (deg C) and latitude in radians (:51-130)."""
    ctx = _hip.get_context(device)
    tas = np.asarray(tas, dtype=np.float64)
    ncell, nmonths = tas.shape
    if nmonths != 12 * (end_yr - start_yr + 1):
        raise ValueError('tas has {} months, {}..{} has {}'.format(nmonths, start_yr, end_yr, 12 * (end_yr - start_yr + 1)))
    bufs = [ctx.upload(tas), ctx.upload(np.asarray(lat_radians, dtype=np.float64).reshape(-1))]
    d_pet = thornthwaite_device(ctx, ncell, nmonths, start_yr, bufs[0], bufs[1], daylight=daylight)
    out = d_pet.download()
    for b in bufs + [d_pet]:
        b.free()
    return out
