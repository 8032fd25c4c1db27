"""Month tables for the harness (host logic).

``set_month_arrays`` mirrors xanthos/utils/general.py:15-50: rows of [year, month_index, days] where a year is
leap iff ``year % 4 == 0`` (general.py:37 -- not the Gregorian rule; the routing sub-step count depends on it,
components.py:276,288).  Penman-Monteith's own calendar (calendar.isleap, penman_monteith.py:57) is applied inside
the PM kernel.
"""
import numpy as np

_DAYS = np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])


def set_month_arrays(n_months, start_year, end_year):
    years = np.repeat(np.arange(start_year, end_year + 1), 12)
    mths = np.tile(np.arange(12), end_year - start_year + 1)
    days = _DAYS[mths] + ((mths == 1) & (years % 4 == 0))
    tab = np.stack([years, mths, days], axis=1).astype(int)
    if tab.shape[0] != n_months:
        raise ValueError('n_months = {} does not match {}..{}'.format(n_months, start_year, end_year))
    return tab


# first and last day of year (1-based) of each month (general.py:74-83)
_MONTH_FIRST = {False: (1, 32, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335),
                True: (1, 32, 61, 92, 122, 153, 183, 214, 245, 275, 306, 336)}
_MONTH_LAST = {False: (31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334, 365),
               True: (31, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335, 366)}


def calc_sinusoidal_factor(yr_imth_ndays, startmonth=1):
    """Solar declination (radians) and inverse relative Earth-Sun distance of each row of a ``set_month_arrays`` table
    (general.py:53-90): the daily values 0.409 sin(2 pi j / n - 1.39 + ph) and 1 + 0.033 cos(2 pi j / n + ph), j = 1..n,
    n = 366 in years with ``year % 4 == 0`` and 365 otherwise, averaged (np.mean) over the days of the month.  Only 24
    distinct (leap, month) pairs exist; each is evaluated once."""
    tab = np.asarray(yr_imth_ndays)
    ph = (startmonth - 1.) / 12. * 2. * np.pi
    cache = {}
    for leap in (False, True):
        j = np.arange(1, 367 if leap else 366)
        arg = 2 * np.pi * j / max(j)
        dec_day = 0.409 * np.sin(arg - 1.39 + ph)
        dr_day = 1. + 0.033 * np.cos(arg + ph)
        for k in range(12):
            sl = slice(_MONTH_FIRST[leap][k] - 1, _MONTH_LAST[leap][k])
            cache[leap, k] = (np.mean(dec_day[sl]), np.mean(dr_day[sl]))
    solar_dec = np.zeros(tab.shape[0])
    dr = np.zeros(tab.shape[0])
    for i in range(tab.shape[0]):
        solar_dec[i], dr[i] = cache[bool(np.mod(tab[i, 0], 4) == 0), int(tab[i, 1])]
    return solar_dec, dr
