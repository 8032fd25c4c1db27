"""The three simple PET stages restated in numpy, in float64 or long double, with a record of every decision per element:

    hargreaves    xanthos/pet/hargreaves.py:17-73 with the harness's preparation (nan_to_num of T and D, negative D -> 0)
    hs            xanthos/pet/hargreaves_samani.py:31-65, :113-114
    daylight      xanthos/pet/thornthwaite.py:18-44
    thornthwaite  xanthos/pet/thornthwaite.py:47-130, and the `monthly` daylight order of csrc/xh_pet_ext.hip

np.float64 is the restatement the device kernels are held to in bits where no transcendental decides an output;
np.longdouble (x86 extended) is the truth the tolerance tests measure against.  The reference's constants enter as the
float64 values the reference uses (np.pi, 0.4102, 0.409, 1.39, 17.8, ...): only the arithmetic and the functions are wider.

Summation order.  The device sums the heat index I (12 months) and the monthly daylight (28-31 days) sequentially; numpy's
np.add.reduceat adds with eight accumulators.  ``order='seq'`` is the device's order, ``order='numpy'`` calls reduceat as
the reference does; the two differ in the last bits of about half of all rows, so only the second is compared with the
reference's outputs, and neither is compared in bits with the device.

``hook = (name, k)`` moves the float64 results of one named transcendental k ulp (k = +-1): 'tan', 'cos', 'sin' (of the
latitude), 'acos', 'sin_acs' (the sine of the sunset angle) and 'pow'.  A correct float64 evaluation with another libm lands
anywhere in that family; tests/pet_cases.py takes the worst of it as E_host.

Every function returns (values, rec): rec.branch the branch code per element, rec.gap the distance to the nearest
discontinuity or singular point (1 - |tn|, 1 - |arg|, the smallest 1 - |x_d| of a month's days, as magnitudes), rec.scale
the error scale in mm (hours for daylight) that errors are divided by.
"""
import calendar
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, 'long double must be x86 extended precision (64-bit mantissa) or wider'

HOOK_NAMES = {'hargreaves': ('tan', 'cos', 'sin', 'acos', 'sin_acs'), 'hs': ('tan', 'cos', 'acos', 'sin_acs'),
              'daylight': ('tan', 'acos'), 'thornthwaite': ('tan', 'acos', 'pow')}
DBL_MAX = np.finfo(np.float64).max
TINY = 2.0 ** -1022                       # below this float64 has no relative precision: the floor of every scale
MONTHDAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
LEAP_MONTHDAYS = (31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
HS_MIDDAY = np.array([15, 45, 75, 105, 135, 165, 195, 225, 255, 285, 315, 345])

# branch codes
HG_IN, HG_BELOW, HG_ABOVE, HG_NAN = 0, 1, 2, 3             # arg in [-1, 1] | arg < -1 (ws = pi) | arg > 1 (ws = 0) | NaN (ws = 0)
HG_NEG_D, HG_NEG_EVAP = 8, 16                              # flags: D < 0 was zeroed; evap < 0 was clipped
HG_MASK = 7
HS_COLD, HS_IN, HS_BELOW, HS_ABOVE, HS_NAN = 0, 1, 2, 3, 4  # t < 0 | tn in [-1, 1] | tn < -1 | tn > 1 | tn NaN
TR_ZERO_I, TR_ZERO_T, TR_WARM = 0, 1, 2                    # I == 0 | t == 0 in a year with I != 0 | t > 0
TR_LEAP = 4                                                # flag: the year takes the leap table


def hooks(stage):
    return [None] + [(n, k) for n in HOOK_NAMES[stage] for k in (1, -1)]


def _tr(name, fn, x, hook):
    with np.errstate(all='ignore'):
        y = fn(x)
    if hook is not None and hook[0] == name:
        assert y.dtype == np.float64, 'hooks move float64 results only'
        # a result of exactly 0 or inf (pow(0, a), acos(1), sin(0), pow(inf, a)) is exact in every libm and stays
        y = np.where((y == 0) | np.isinf(y), y, np.nextafter(y, np.inf if hook[1] > 0 else -np.inf))
    return y


def _nan_to_num(a, T):
    a = np.asarray(a, dtype=np.float64)
    a = np.where(a != a, 0.0, np.where(a == np.inf, DBL_MAX, np.where(a == -np.inf, -DBL_MAX, a)))
    return a.astype(T)


def _c_phi(phi):
    """1 + |phi| / |sin phi cos phi|: the relative change of tan(phi) per relative change of phi, plus one for the factor
    tan(declination).  2 at phi = 0 (the limit)."""
    with np.errstate(all='ignore'):
        c = 1 + np.abs(phi) / np.abs(np.sin(phi) * np.cos(phi))
    return np.where(phi == 0, 2, c)


# ------------------------------------------------------------------------------------------------------- Hargreaves
def hargreaves(temp, dtr, lat, dec, dr, ndays, dtype=np.float64, hook=None):
    """temp, dtr [ncell, nmonths]; lat [ncell] in radians; dec, dr, ndays [nmonths] (month_factors)."""
    T = dtype
    t, d = _nan_to_num(temp, T), _nan_to_num(dtr, T)               # components.py:156-157, :178-179
    neg = d < 0
    d = np.where(neg, T(0), d)                                     # data_load.py:83-84, hargreaves.py:32
    X = np.asarray(lat, dtype=np.float64).astype(T)[:, None]
    Y, dr, nd = (np.asarray(a, dtype=np.float64).astype(T)[None, :] for a in (dec, dr, ndays))
    with np.errstate(all='ignore'):
        sx, cx, tx = _tr('sin', np.sin, X, hook), _tr('cos', np.cos, X, hook), _tr('tan', np.tan, X, hook)
        arg = -tx * np.tan(Y)                                      # :50
        inside = (arg <= 1) & (arg >= -1)                          # :64
        ws = np.where(inside, _tr('acos', np.arccos, np.where(inside, arg, T(0)), hook),
                      np.where(arg < -1, T(np.pi), T(0)))          # :67-71; NaN matches none and stays 0
        a = ws * sx * np.sin(Y)
        b = cx * np.cos(Y) * _tr('sin_acs', np.sin, ws, hook)
        ra = T(15.392) * dr * (a + b)                              # :44
        evap = nd * T(0.0023) * ra * (t + T(17.8)) * np.sqrt(d)    # :35
        low = evap < 0
        out = np.where(low, T(0), evap)                            # np.maximum(evap, 0): NaN stays NaN
        branch = np.where(inside, HG_IN, np.where(arg < -1, HG_BELOW, np.where(arg > 1, HG_ABOVE, HG_NAN)))
        branch = np.broadcast_to(branch, out.shape) | (neg * HG_NEG_D) | (low * HG_NEG_EVAP)
        gap = np.broadcast_to(np.abs(1 - np.abs(arg)), out.shape)
        scale = nd * T(0.0023) * T(15.392) * dr * (np.abs(a) + np.abs(b)) * (np.abs(t) + T(17.8)) * np.sqrt(d)
    return out, SimpleNamespace(branch=branch.astype(np.int32), gap=gap, scale=scale, arg=arg)


# ------------------------------------------------------------------------------------------------------- Hargreaves-Samani
def hs_delta(nmonths, T):
    """hargreaves_samani.py:39-48: the declination of the middle of month mth % 12."""
    dy = HS_MIDDAY[np.arange(nmonths) % 12]
    return T(0.4102) * np.sin(2 * (T(np.pi) / 365) * (dy - 80).astype(T))


def hs(tas, tmax, tmin, lat_deg, ndays, dtype=np.float64, hook=None):
    """tas, tmax, tmin [ncell, nmonths]; lat_deg [ncell]; ndays [nmonths].  mm/month."""
    T = dtype
    t, tx, tm = (np.asarray(a, dtype=np.float64).astype(T) for a in (tas, tmax, tmin))
    nd = np.asarray(ndays, dtype=np.float64).astype(T)[None, :]
    pi = T(np.pi)
    delta = hs_delta(t.shape[1], T)[None, :]
    phi = np.asarray(lat_deg, dtype=np.float64).astype(T)[:, None] * pi / 180           # :50
    with np.errstate(all='ignore'):
        cphi, tphi = _tr('cos', np.cos, phi, hook), _tr('tan', np.tan, phi, hook)
        tn = -np.tan(delta) * tphi                                 # :52
        outside = (tn < -1) | (tn > 1)                             # :54
        acs = np.where(outside, T(0), _tr('acos', np.arccos, np.where(outside, T(0), tn), hook))
        ra = T(118) / pi * acs + cphi * np.cos(delta) * _tr('sin_acs', np.sin, acs, hook)       # :60
        k = T(0.408) * T(0.0023)
        p = k * ra * (t + T(17.8)) * np.sqrt(np.abs(tx - tm))     # :63
        cold = t < 0                                               # :33 (NaN is not < 0)
        out = np.where(cold, T(0), p * nd)                         # :114
        branch = np.where(tn < -1, HS_BELOW, np.where(tn > 1, HS_ABOVE, np.where(tn != tn, HS_NAN, HS_IN)))
        branch = np.where(cold, HS_COLD, np.broadcast_to(branch, out.shape))
        gap = np.broadcast_to(np.abs(1 - np.abs(tn)), out.shape)
        K = k * (np.abs(t) + T(17.8)) * np.sqrt(np.abs(tx - tm)) * nd
        dra = T(118) / pi + np.abs(cphi * np.cos(delta) * np.cos(acs))
        sens = np.where(outside, T(0), dra * np.abs(tn) * _c_phi(phi) / np.sqrt(np.abs(1 - tn * tn)))
        scale = np.where(cold, T(0), K * (np.abs(ra) + sens))
    return out, SimpleNamespace(branch=branch.astype(np.int32), gap=gap, scale=scale, tn=np.broadcast_to(tn, out.shape))


# ------------------------------------------------------------------------------------------------------- daylight
def _month_sums(v, mth_days, order):
    """Sums of consecutive runs of mth_days columns: one after the other (the device) or by np.add.reduceat (numpy)."""
    idx = np.concatenate([[0], np.cumsum(mth_days)[:-1]])
    if order == 'numpy':
        return np.add.reduceat(v, idx, axis=1)
    out = np.zeros((v.shape[0], len(mth_days)), dtype=v.dtype)
    for k, (i, n) in enumerate(zip(idx, mth_days)):
        for d in range(i, i + n):
            out[:, k] = out[:, k] + v[:, d]
    return out


def daylight(lat, leap, dtype=np.float64, hook=None, order='seq'):
    """Mean daylight hours [ncell, 12] of the months of a common (leap = False) or a leap year; lat in radians."""
    T = dtype
    mth_days = LEAP_MONTHDAYS if leap else MONTHDAYS
    day = (np.arange(sum(mth_days)) + 1).astype(T)
    X = np.asarray(lat, dtype=np.float64).astype(T)[:, None]
    with np.errstate(all='ignore'):
        dec = T(0.409) * np.sin((2 * T(np.pi) / T(365.0)) * day - T(1.39))             # :31
        x = -_tr('tan', np.tan, X, hook) * np.tan(dec)[None, :]                        # :35
        xc = np.where(x < -1, T(-1), np.where(x > 1, T(1), x))                          # np.clip: NaN stays NaN
        hours = _tr('acos', np.arccos, xc, hook) * (T(24.0) / T(np.pi))                # :36, :39
        out = _month_sums(hours, mth_days, order) / np.array(mth_days).astype(T)       # :42
        idx = np.concatenate([[0], np.cumsum(mth_days)[:-1]])
        lo = np.add.reduceat((x < -1).astype(np.int32), idx, axis=1)
        hi = np.add.reduceat((x > 1).astype(np.int32), idx, axis=1)
        g = np.abs(1 - np.abs(x))
        g = np.where(g == g, g, T(np.inf))
        gap = np.minimum.reduceat(g, idx, axis=1)
        # 24 h, and the first-order sensitivity of every unclipped day to its argument: d acos = dx / sqrt(1 - x^2), with
        # dx / x = c_phi roundings (the tangent of the latitude amplifies its own rounding towards the poles)
        free = (x >= -1) & (x <= 1) & (np.abs(x) != 1)
        sens = np.where(free, np.abs(x) * _c_phi(X) / np.sqrt(np.abs(1 - np.where(free, x, T(0)) ** 2)), T(0))
        scale = T(24.0) + T(24.0) / T(np.pi) * np.add.reduceat(sens, idx, axis=1) / np.array(mth_days).astype(T)
    # branch: how many of the month's days are clipped below and above (a NaN latitude: -1)
    branch = np.where(np.isnan(out), -1, lo * 64 + hi).astype(np.int32)
    return out, SimpleNamespace(branch=branch, gap=gap, scale=scale, lo=lo, hi=hi, x=x)


# ------------------------------------------------------------------------------------------------------- Thornthwaite
def isleap(y):
    return calendar.isleap(int(y))


def daylight_columns(nyears, y, leap, monthly):
    """The column of the [ncell, 24] table (12 common months, 12 leap) that year y of the run reads for its 12 months:
    np.repeat(L, nyears, axis=1) gives global month m of a common year column m // nyears (thornthwaite.py:110)."""
    k = np.arange(12)
    return 12 + k if leap else (k if monthly else (12 * y + k) // nyears)


def thornthwaite(tas, lat, y0, y1, monthly=False, dtype=np.float64, hook=None, order='seq'):
    """tas [ncell, 12 nyears]; lat [ncell] in radians.  mm/month."""
    T = dtype
    ny = y1 - y0 + 1
    v = np.asarray(tas, dtype=np.float64)
    assert v.shape[1] == 12 * ny
    t = np.where((v != v) | (v < 0), 0.0, v).astype(T)                                 # :82
    with np.errstate(all='ignore'):
        i = _tr('pow', lambda z: np.power(z, T(1.514)), t / T(5.0), hook)              # :88
        if order == 'numpy':
            I = np.add.reduceat(i, np.arange(0, i.shape[1], 12), axis=1)               # :91
        else:
            I = np.zeros((t.shape[0], ny), dtype=T)
            for k in range(12):
                I = I + i[:, k::12]
        terms = [T(.000000675) * _tr('pow', lambda z: np.power(z, T(3)), I, hook), T(.0000771) * (I * I), T(.0179) * I,
                 T(.492) * np.ones_like(I)]
        a = terms[0] - terms[1] + terms[2] + terms[3]                                  # :94
        asum = np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2]) + np.abs(terms[3])
        I12, a12, asum12 = (np.repeat(z, 12, axis=1) for z in (I, a, asum))            # :97-98
        q = np.where(I12 != 0, 10 * t / np.where(I12 != 0, I12, T(1)), T(0))           # :104
        pu = 16 * _tr('pow', lambda z: np.power(z, a12), q, hook)                      # :105
        two = [daylight(lat, leap, T, hook, order) for leap in (False, True)]
        dl = np.concatenate([two[0][0], two[1][0]], axis=1)
        dl_scale = np.concatenate([two[0][1].scale, two[1][1].scale], axis=1)
        dl_gap = np.concatenate([two[0][1].gap, two[1][1].gap], axis=1)
        leap = np.array([isleap(y) for y in range(y0, y1 + 1)])
        cols = np.concatenate([daylight_columns(ny, y, leap[y], monthly) for y in range(ny)])
        L = dl[:, cols]                                                                # :109-119
        N = np.array([LEAP_MONTHDAYS if ly else MONTHDAYS for ly in leap]).flatten().astype(T)          # :122
        out = pu * (L / 12) * (N / T(30.0))                                            # :127
        branch = np.where(I12 == 0, TR_ZERO_I, np.where(t == 0, TR_ZERO_T, TR_WARM)) | (np.repeat(leap, 12)[None, :] * TR_LEAP)
        # |PET| x (1 + a + |ln(10 t / I)| x the magnitudes of a's four terms), and the daylight's own error, which is
        # relative to the daylight's scale (24 h and more) and not to L: pu x scale_L / 12 x N / 30
        cond = 1 + np.abs(a12) + np.abs(np.log(np.where(q > 0, q, T(1)))) * asum12
        scale = np.abs(pu) * (N / T(30.0)) * (np.abs(L) * cond + dl_scale[:, cols]) / 12
        scale = np.where(q > 0, scale, T(0))
    return out, SimpleNamespace(branch=branch.astype(np.int32), scale=scale, I=I, a=a, daylight=dl, cols=cols, N=N,
                                gap=dl_gap[:, cols])


# ------------------------------------------------------------------------------------------------------- comparison
def classes_equal(x, host):
    """The NaN, inf (with sign) and zero masks of x are those of the float64 restatement."""
    x, host = np.asarray(x), np.asarray(host)
    return (np.array_equal(np.isnan(x), np.isnan(host)) and np.array_equal(np.isinf(x), np.isinf(host))
            and np.array_equal(x[np.isinf(host)] > 0, host[np.isinf(host)] > 0) and np.array_equal(x == 0, host == 0))


def errors(x, truth, scale, host):
    """|x - truth| / scale per element where the float64 restatement ``host`` is finite (elsewhere the expectation is the
    restatement's class, and the error counts 0).  The scale has the floor TINY; where it is 0 the output is decided
    without arithmetic and any difference counts as infinite."""
    x, truth, scale, host = (np.asarray(a) for a in (x, truth, scale, host))
    fin = np.isfinite(host) & np.isfinite(x)
    with np.errstate(all='ignore'):
        d = np.abs(np.where(fin, x, 0).astype(LD) - np.where(fin, truth, 0))
        e = np.where(scale > 0, d / np.maximum(scale, LD(TINY)), np.where(d == 0, LD(0), LD(np.inf)))
    return np.where(fin, e, LD(0))


def same(x, y):
    """Equal as numbers, element by element; a NaN equals any NaN."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and bool(np.all((x == y) | (np.isnan(x) & np.isnan(y))))


def same_bits(x, y):
    """Equal bit for bit, the sign of zero included; a NaN equals any NaN."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and bool(np.all((x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))))
