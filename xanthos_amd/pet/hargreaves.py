"""Hargreaves monthly PET -- drop-in for xanthos/pet/hargreaves.py on MI355X.

Same plugin entry point as the reference (components.py:193-195), one month per call:

    calculate_pet(temp, dtr, x, y, dr, m) -> [ncell]

plus ``hargreaves_device`` / ``run_hargreaves`` for the whole series in one launch (csrc/xh_gwam.hip, k_hargreaves_pet).
The input preparation the reference spreads over the loader and the harness -- negative DTR -> 0 (data_load.py:83-84,
hargreaves.py:33) and nan_to_num of T and D (components.py:144-187) -- happens in the kernel.  Unlike the reference,
``calculate_pet`` does not zero the negative entries of the caller's ``dtr`` in place.
"""
import numpy as np

from .. import _hip
from ..utils import calc_sinusoidal_factor, set_month_arrays


def month_factors(start_year, end_year):
    """(solar declination, dr, days) per month of the run (general.py:15-90)."""
    nmonths = (end_year - start_year + 1) * 12
    tab = set_month_arrays(nmonths, start_year, end_year)
    dec, dr = calc_sinusoidal_factor(tab)
    return dec, dr, tab[:, 2].astype(np.float64)


def hargreaves_device(ctx, ncell, nmonths, d_temp, d_dtr, d_lat, solar_dec, dr, ndays, d_pet=None):
    """Device-resident variant: d_* are DeviceArrays in HBM; returns the PET DeviceArray [ncell, nmonths]."""
    if d_pet is None:
        d_pet = ctx.empty((ncell, nmonths))
    ctx.hargreaves_pet(ncell, nmonths, d_temp, d_dtr, d_lat, solar_dec, dr, ndays, d_pet)
    return d_pet


def run_hargreaves(temp, dtr, lat_radians, start_year, end_year, device=0):
    """PET [ncell, nmonths] of the whole series from host arrays (the reference's step loop, components.py:325-340)."""
    ctx = _hip.get_context(device)
    temp = np.asarray(temp, dtype=np.float64)
    ncell, nmonths = temp.shape
    dec, dr, nd = month_factors(start_year, end_year)
    if nmonths != dec.size:
        raise ValueError('temperature has {} months, {}..{} has {}'.format(nmonths, start_year, end_year, dec.size))
    bufs = [ctx.upload(temp), ctx.upload(np.asarray(dtr, dtype=np.float64)),
            ctx.upload(np.asarray(lat_radians, dtype=np.float64).reshape(-1))]
    d_pet = hargreaves_device(ctx, ncell, nmonths, bufs[0], bufs[1], bufs[2], dec, dr, nd)
    out = d_pet.download()
    for b in bufs + [d_pet]:
        b.free()
    return out


def calculate_pet(temp, dtr, x, y, dr, m, device=0):
    """PET of one month, mm/month (hargreaves.py:17-41): temp, dtr [ncell]; x latitude [ncell] in radians; y solar
    declination, dr inverse relative Earth-Sun distance and m days of the month (scalars)."""
    ctx = _hip.get_context(device)
    temp = np.asarray(temp, dtype=np.float64).reshape(-1)
    ncell = temp.size
    bufs = [ctx.upload(temp), ctx.upload(np.asarray(dtr, dtype=np.float64).reshape(-1)),
            ctx.upload(np.asarray(x, dtype=np.float64).reshape(-1))]
    d_pet = hargreaves_device(ctx, ncell, 1, bufs[0], bufs[1], bufs[2], [float(y)], [float(dr)], [float(m)])
    out = d_pet.download().reshape(-1)
    for b in bufs + [d_pet]:
        b.free()
    return out
