"""The test inputs of the three simple PET stages (Hargreaves, Hargreaves-Samani, Thornthwaite with its daylight table), the
long-double truth, and the bar a correct float64 evaluation sets.  Shared by tests/test_pet_edges_host.py,
tests/test_gpu_pet_edges.py and tests/golden/make_golden_pet_edges.py.

Set A holds the edges.  Its latitudes are 0, the poles as float64 and their neighbours one ulp inside, NaN, and -- for each
of the 12 months of the two Hargreaves stages and for days 1, 172 and 355 of the daylight table -- the eight latitudes that
put the sunset argument at 1 -+ m and -1 +- m, m = 1e-3 and 1e-6, solved in long double and rounded.  A case is one
(cell, month) element; so that a call has the shape the ABI takes, cells are latitudes and the other inputs change from
month to month:

  Hargreaves  102 latitudes x 3 cells x 36 months (month_factors(1899, 1901)): one cell with T = 20, D = 12 throughout, two
              walking through the 10 x 9 products of T_VALUES and D_VALUES, so that every product meets every branch
  HS          102 latitudes x 2 cells x 48 months (the days of 1899-1901 and of 2000; months >= 12 go through m % 12): one cell
              with tas = 30, one walking through TAS_VALUES; (tmax, tmin) ordinary, equal, reversed, NaN in either
  daylight    30 latitudes x 24 (common and leap year)
  Thornthwaite  9 year patterns x 8 latitudes, as one-year runs from each of YEARS_A (leap by % 4, not by % 100, by % 400)

Set B holds grids: 181 latitudes (-90 ... 90 degrees) x the 24 months of 1899-1900 with seeded T and D for the Hargreaves pair,
the same latitudes for daylight, and 300 cells x nyears in NYEARS_B from 1896 (leap), through 1900 (not) and 1904 (leap) in both
daylight orders for Thornthwaite.

``truth(stage, set, ...)`` evaluates a run in long double and in float64 under every one-ulp nudge of tests/pet_np.py;
``bar(stage, set)`` is 4 x E_host, E_host the worst |float64 - truth| / scale over the set's runs and nudges.  A case is
left out of the bar only if its gap to a discontinuity is below NEAR and not exactly 0; tests/test_pet_edges_host.py asserts
that no case of either set is, and that no branch differs between the float64 and the long-double record.
"""
import calendar
from types import SimpleNamespace

import numpy as np

import pet_np as P
from pet_np import LD

NEAR = 1e-9
BAR_FACTOR = 4.0
MARGINS = (1e-3, 1e-6)
NAN, INF = float('nan'), float('inf')

T_VALUES = (-40.0, -17.8, np.nextafter(-17.8, 0), np.nextafter(-17.8, -100), -0.0, 0.0, 45.0, NAN, INF, -INF)
D_VALUES = (-INF, -3.0, -0.0, 0.0, 5e-324, 1e-300, 12.0, INF, NAN)
TAS_VALUES = (-5e-324, -0.0, 0.0, 5e-324, -1.0, 30.0, NAN, INF)
ORDERINGS = ('ordinary', 'equal', 'reversed', 'tmax NaN', 'tmin NaN')
YEARS_A = (1896, 1900, 1904, 2000, 2100, 2400)
NYEARS_B = (1, 2, 3, 5, 7, 12, 13)
Y0_B = 1896
DAYS_A = (1, 172, 355)
SEED = 11


def _targets():
    """(label, sunset argument) on both sides of +1 and of -1."""
    return [('{:+d}{}{:g}'.format(s, '-' if inner else '+', m), s * (1 - m if inner else 1 + m))
            for s in (1, -1) for m in MARGINS for inner in (True, False)]


def _edge_latitudes(pole, tans, names, to_lat):
    """0, the poles, their neighbours one ulp inside, NaN, then for every tangent of a declination in ``tans`` the latitudes
    with -tan(lat) tan(dec) = target.  ``to_lat`` maps radians (long double) to the stage's unit."""
    lab = ['lat 0', 'pole N', 'pole S', 'pole N inside', 'pole S inside', 'lat NaN']
    lat = [0.0, pole, -pole, np.nextafter(pole, 0), np.nextafter(-pole, 0), NAN]
    for name, td in zip(names, tans):
        for tl, target in _targets():
            lab.append('{} arg {}'.format(name, tl))
            lat.append(float(to_lat(np.arctan(-LD(target) / td))))
    return np.array(lab), np.array(lat, dtype=np.float64)


def month_factors(y0, y1):
    from xanthos_amd.pet.hargreaves import month_factors as mf
    return mf(y0, y1)


def days(years):
    return np.array([calendar.monthrange(y, m)[1] for y in years for m in range(1, 13)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------- the case sets
def hg_a():
    dec, dr, nd = month_factors(1899, 1901)
    lab, lat = _edge_latitudes(np.pi / 2, np.tan(dec[:12].astype(LD)), ['month {}'.format(k) for k in range(12)], lambda x: x)
    nl, nm = lat.size, dec.size
    combos = [(t, d) for t in T_VALUES for d in D_VALUES]
    li, m = np.arange(nl)[:, None], np.arange(nm)[None, :]
    walk = [(li * 36 + m) % len(combos), (li * 36 + m + 45) % len(combos)]
    tv, dv = np.array([c[0] for c in combos]), np.array([c[1] for c in combos])
    temp = np.concatenate([np.full((nl, nm), 20.0), tv[walk[0]], tv[walk[1]]])
    dtr = np.concatenate([np.full((nl, nm), 12.0), dv[walk[0]], dv[walk[1]]])
    return SimpleNamespace(label=np.tile(lab, 3), lat=np.tile(lat, 3), temp=temp, dtr=dtr, dec=dec, dr=dr, nd=nd)


def hg_b():
    rng = np.random.default_rng(SEED)
    dec, dr, nd = month_factors(1899, 1900)
    lat = np.radians(np.arange(-90.0, 91.0))
    temp = rng.uniform(-45, 40, (lat.size, 24))
    dtr = rng.uniform(-2, 20, (lat.size, 24))
    return SimpleNamespace(label=np.full(lat.size, 'grid'), lat=lat, temp=temp, dtr=dtr, dec=dec, dr=dr, nd=nd)


def _orderings(tas, which):
    base = np.where(np.isfinite(tas), tas, 10.0)
    tmax = np.select([which == 0, which == 1, which == 2, which == 3, which == 4], [base + 6, base + 3, base - 5, NAN, base + 6])
    tmin = np.select([which == 0, which == 1, which == 2, which == 3, which == 4], [base - 5, base + 3, base + 6, base - 5, NAN])
    return tmax, tmin


def hs_a():
    nd = days((1899, 1900, 1901, 2000))
    tdelta = np.tan(P.hs_delta(12, LD))
    lab, lat = _edge_latitudes(90.0, tdelta, ['month {}'.format(k) for k in range(12)], lambda x: x * 180 / LD(np.pi))
    nl, nm = lat.size, nd.size
    li, m = np.arange(nl)[:, None], np.arange(nm)[None, :]
    tas = np.concatenate([np.full((nl, nm), 30.0), np.array(TAS_VALUES)[(li + m) % len(TAS_VALUES)]])
    which = np.concatenate([(li + m // 12) % 5, ((li * 3 + m) // 8) % 5])
    tmax, tmin = _orderings(tas, which)
    return SimpleNamespace(label=np.tile(lab, 2), lat=np.tile(lat, 2), tas=tas, tmax=tmax, tmin=tmin, nd=nd, ordering=which)


def hs_b():
    rng = np.random.default_rng(SEED + 1)
    lat = np.arange(-90.0, 91.0)
    tas = rng.uniform(-10, 35, (lat.size, 24))
    tmin, tmax = tas - rng.uniform(0, 15, tas.shape), tas + rng.uniform(0, 15, tas.shape)
    return SimpleNamespace(label=np.full(lat.size, 'grid'), lat=lat, tas=tas, tmax=tmax, tmin=tmin, nd=days((1899, 1900)),
                           ordering=np.zeros(tas.shape, dtype=int))


def _tan_dec_day(d):
    return np.tan(LD(0.409) * np.sin((2 * LD(np.pi) / LD(365.0)) * LD(d) - LD(1.39)))


def dl_a():
    lab, lat = _edge_latitudes(np.pi / 2, [_tan_dec_day(d) for d in DAYS_A], ['day {}'.format(d) for d in DAYS_A], lambda x: x)
    return SimpleNamespace(label=lab, lat=lat)


def dl_b():
    lat = np.radians(np.arange(-90.0, 91.0))
    return SimpleNamespace(label=np.full(lat.size, 'grid'), lat=lat)


WARM = (4.0, 6.5, 9.0, 13.0, 17.5, 21.0, 24.5, 23.0, 19.0, 14.0, 8.5, 5.0)
TR_PATTERNS = [
    ('all negative', tuple(-5.0 - k for k in range(12))),                  # I == 0
    ('all NaN', (NAN,) * 12),                                              # NaN counts as 0: I == 0, PET 0
    ('one warm among cold', (-3.0,) * 6 + (18.0,) + (-3.0,) * 5),
    ('one zero among warm', WARM[:3] + (0.0,) + WARM[4:]),
    ('40 throughout', (40.0,) * 12),
    ('denormal month', WARM[:8] + (5e-324,) + WARM[9:]),
    ('inf month', WARM[:5] + (INF,) + WARM[6:]),
    ('negative zero month', WARM[:10] + (-0.0,) + WARM[11:]),
    ('ordinary', WARM),
]
TR_LATS_A = (0.0, 0.698132, -0.9, 1.3, np.pi / 2, -np.pi / 2, np.nextafter(np.pi / 2, 0), NAN)


def tr_a():
    """72 cells of one year; run once from each start year of YEARS_A."""
    tas = np.array([p[1] for p in TR_PATTERNS for _ in TR_LATS_A], dtype=np.float64)
    lab = np.array([p[0] for p in TR_PATTERNS for _ in TR_LATS_A])
    return SimpleNamespace(label=lab, lat=np.array(TR_LATS_A * len(TR_PATTERNS), dtype=np.float64), tas=tas)


NC_TR_B = 300


def tr_b(nyears=max(NYEARS_B)):
    """300 cells x nyears; shorter runs are prefixes of the 13-year forcing."""
    rng = np.random.default_rng(SEED + 2)
    tas = rng.uniform(-15, 40, (NC_TR_B, 12 * max(NYEARS_B)))
    lat = np.radians(rng.uniform(-90, 90, NC_TR_B))
    lat[:4] = np.pi / 2, -np.pi / 2, 0.0, np.radians(66.0)
    return SimpleNamespace(label=np.full(NC_TR_B, 'grid'), lat=lat, tas=np.ascontiguousarray(tas[:, :12 * nyears]))


GOLDEN_B_LATS = slice(None, None, 4)                       # the rows of the latitude grids whose reference outputs are kept
GOLDEN_B_CELLS = slice(0, 10)                              # the cells of Thornthwaite's set B


# ------------------------------------------------------------------------------------------------------- truth and bar
_cache = {}
CASES = {('hg', 'a'): hg_a, ('hg', 'b'): hg_b, ('hs', 'a'): hs_a, ('hs', 'b'): hs_b, ('dl', 'a'): dl_a, ('dl', 'b'): dl_b,
         ('tr', 'a'): tr_a}
STAGE = {'hg': 'hargreaves', 'hs': 'hs', 'dl': 'daylight', 'tr': 'thornthwaite'}


def cases(stage, which, *key):
    k = ('cases', stage, which) + key
    if k not in _cache:
        _cache[k] = tr_b(*key) if (stage, which) == ('tr', 'b') else CASES[stage, which]()
    return _cache[k]


def runs(stage, which):
    """The keys of the runs a set consists of."""
    if stage == 'tr':
        return [(y,) for y in YEARS_A] if which == 'a' else [(ny, mo) for ny in NYEARS_B for mo in (False, True)]
    return [()]


def _both_tables(lat, T, hook, order):
    a, ra = P.daylight(lat, False, T, hook, order)
    b, rb = P.daylight(lat, True, T, hook, order)
    cat = lambda x, y: np.concatenate([x, y], axis=1)                      # noqa: E731
    return cat(a, b), SimpleNamespace(branch=cat(ra.branch, rb.branch), gap=cat(ra.gap, rb.gap), scale=cat(ra.scale, rb.scale),
                                      lo=cat(ra.lo, rb.lo), hi=cat(ra.hi, rb.hi))


def runner(stage, which, *key):
    """f(dtype, hook, order='seq') -> (values, rec) of one run."""
    if stage == 'hg':
        cs = cases(stage, which)
        return cs, lambda T, hook, order='seq': P.hargreaves(cs.temp, cs.dtr, cs.lat, cs.dec, cs.dr, cs.nd, T, hook)
    if stage == 'hs':
        cs = cases(stage, which)
        return cs, lambda T, hook, order='seq': P.hs(cs.tas, cs.tmax, cs.tmin, cs.lat, cs.nd, T, hook)
    if stage == 'dl':
        cs = cases(stage, which)
        return cs, lambda T, hook, order='seq': _both_tables(cs.lat, T, hook, order)
    if which == 'a':
        cs, y0, y1, monthly = cases('tr', 'a'), key[0], key[0], False
    else:
        cs, y0, y1, monthly = cases('tr', 'b', key[0]), Y0_B, Y0_B + key[0] - 1, key[1]
    return cs, lambda T, hook, order='seq': P.thornthwaite(cs.tas, cs.lat, y0, y1, monthly, T, hook, order)


def truth(stage, which, *key):
    """One run in long double: .cs, .truth, .rec, .hosts [(values, rec) of the float64 restatement, plain first, then each
    one-ulp nudge], .host (the plain values), .scale, .left_out, .e_host (of this run)."""
    k = ('truth', stage, which) + key
    if k not in _cache:
        cs, f = runner(stage, which, *key)
        t, rec = f(LD, None)
        hosts = [f(np.float64, h) for h in P.hooks(STAGE[stage])]
        gap = np.asarray(rec.gap)
        left = (gap != 0) & (gap < NEAR)
        host = hosts[0][0]
        e = max(float(P.errors(h[0], t, rec.scale, host)[~left].max()) for h in hosts)
        _cache[k] = SimpleNamespace(cs=cs, truth=t, rec=rec, hosts=hosts, host=host, scale=rec.scale, left_out=left, e_host=e,
                                    run=f)
    return _cache[k]


def e_host(stage, which):
    return max(truth(stage, which, *key).e_host for key in runs(stage, which))


def bar(stage, which):
    return BAR_FACTOR * e_host(stage, which)


def worst(x, t):
    """The worst error of x, in units of scale, over the cases of run ``t`` that count."""
    return float(P.errors(x, t.truth, t.scale, t.host)[~t.left_out].max())
