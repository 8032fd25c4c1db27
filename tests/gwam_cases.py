"""The GWAM test inputs: case sets A (one month, one case per cell), B (marches of 50 months) and C (shapes), as plain
functions of a seed.  Shared by tests/test_gwam_host.py, tests/test_gpu_gwam.py and tests/golden/make_golden_gwam_edges.py.

Set A is the product of x = ch / Sm, Sm, PET and P over the values below (every factor jittered by +-1e-3 relative, so that
nothing sits on a computed threshold by accident) followed by hand-written blocks: exact ties made of dyadic numbers
(identical in every precision), the branches without arithmetic, and inputs only a file can deliver.  ``label`` names the
block of every cell.

Set B is 1,200 cells x 50 months (50 = 2 mod 16: consecutive cells take all eight row shifts of k_gwam_tile, and a row spans
four tiles), the forcing classes of gwam.npz plus cells whose precipitation is zero in most months; the initial storage is
Sm x one of {0, 0.05, 0.5, 1, 1.3, 2.6}, every class meeting every factor.

Set C names the shapes: (nmonths, ncell) pairs and the cell indices a row of B is placed at.
"""
import itertools
from types import SimpleNamespace

import numpy as np

SEED_A = 20
SEED_B = 7

X_VALUES = (0, 1e-12, 0.01, 0.05, 0.0607, 0.0608, 0.1, 0.3, 0.5, 0.75, 0.999, 1, 1.1, 1.25, 1.5, 1.6, 2.0, 2.44, 2.6)
SM_VALUES = (0.5, 10, 137.3, 500, 4000)
PET_VALUES = (0, 0.3, 5, 60, 250)
P_VALUES = (0, 1e-3, 2, 40, 300, 1500)

NAN, INF = float('nan'), float('inf')

# (label, ch, P, PET, Sm)
HAND = [
    # ---- exact ties from dyadic numbers
    ('tie B == Sm', 1.5, 2.25, 0.75, 3.0),                 # B = 3 = Sm: the full branch, Q = +0
    ('tie B == Sm', 0.0, 8.0, 4.0, 4.0),
    ('tie B == Sm', 6.0, 0.0, 2.0, 4.0),                   # from above capacity (x = 1.5)
    ('tie tmp3 == tmp7', 5.0, 1.0, 6.0, 4.0),              # x = 1.25: tmp5 = 25/24, tmp6 = 1, tmp7 = PET = 6 = ch + P
    ('tie tmp3 == tmp7', 6.0, 0.5, 6.5, 4.0),              # x = 1.5: tmp5 = 1 exactly, tmp7 = PET = ch + P
    ('tie tmp5 == 1', 4.0, 5.0, 7.0, 4.0),                 # x = 1: tmp5 = (5 - 2) / 3 = 1 exactly; tmp7 = PET < tmp3
    ('tie tmp5 == 1', 6.0, 0.25, 4.0, 4.0),                # x = 1.5: tmp5 = (7.5 - 4.5) / 3 = 1 exactly; tmp7 = PET < tmp3
    ('tie P == PET lake', 7.0, 12.5, 12.5, 999.0),
    ('tie P == PET lake', 0.0, 0.0, 0.0, 999.0),
    ('tie ch = P = 0', 0.0, 0.0, 5.0, 100.0),              # tmp3 = 0 <= tmp7; tmp8 = 0: Sav = 0, AET = 0
    ('tie ch = P = 0', 0.0, 0.0, 0.0, 100.0),
    ('tie tmp8 == 0', 0.0, 2.0, 40.0, 100.0),              # ch = 0: tmp8 = P - AET = 0 with AET = tmp3
    ('tie tmp8 == 0', 0.0, 0.75, 64.0, 0.5),
    # ---- the branches without arithmetic
    ('lake NaN', 3.0, NAN, 5.0, 999.0),
    ('lake NaN', 3.0, 5.0, NAN, 999.0),
    ('lake NaN', 3.0, NAN, NAN, 999.0),
    ('lake NaN', NAN, 9.0, 5.0, 999.0),
    ('no soil', 3.0, 4.0, 1.0, 0.0),
    ('no soil', 3.0, 4.0, 1.0, -0.0),
    ('no soil', NAN, NAN, NAN, 0.0),
    ('Sm NaN', 3.0, 4.0, 1.0, NAN),
    ('Sm NaN', 3.0, 400.0, 1.0, NAN),
    ('ch NaN', NAN, 4.0, 1.0, 100.0),
    ('PET NaN soil', 3.0, 4.0, NAN, 100.0),
    ('PET NaN soil', 300.0, 4.0, NAN, 100.0),
    ('P NaN soil', 3.0, NAN, 1.0, 100.0),                  # B is NaN, no branch matches: zeros
    ('P NaN soil', 300.0, NAN, 1.0, 100.0),
    # ---- inputs a file can deliver
    ('inf', 3.0, INF, 5.0, 100.0),                         # full: Q = inf
    ('inf', 3.0, -INF, 5.0, 100.0),                        # partial: AET = -inf, tmp8 = NaN
    ('inf', 3.0, 4.0, INF, 100.0),                         # partial: tmp7 = inf
    ('inf', 3.0, 4.0, -INF, 100.0),                        # full: Q = inf, AET = -inf
    ('inf', 3.0, INF, INF, 100.0),                         # B = NaN
    ('inf', 0.0, 4.0, INF, 100.0),                         # tmp5 = 0: tmp7 = inf x 0.1
    ('inf', 3.0, INF, 5.0, 999.0),
    ('inf', 3.0, -INF, 5.0, 999.0),
    ('inf', 3.0, 4.0, INF, 999.0),
    ('inf', 3.0, 4.0, -INF, 999.0),
    ('inf', 3.0, INF, INF, 999.0),                         # P - PET = NaN -> Q = 0, AET = inf
    ('inf', 3.0, -INF, -INF, 999.0),
    ('inf', INF, 4.0, 5.0, 100.0),                         # a state of inf
    ('negative', 30.0, -2.0, 5.0, 100.0),
    ('negative', 0.0, -2.0, 5.0, 100.0),                   # tmp3 < 0: AET = -2, Sav = 0
    ('negative', 0.5, -2.0, 0.0, 100.0),
    ('negative', 30.0, 4.0, -5.0, 100.0),                  # tmp7 < 0
    ('negative', 99.0, 4.0, -5.0, 100.0),                  # negative PET fills the soil
    ('negative', 30.0, -4.0, -5.0, 100.0),
    ('negative', -3.0, 40.0, 5.0, 100.0),                  # a negative state
    ('negative', 3.0, -2.0, 5.0, 999.0),
    ('negative', 3.0, 2.0, -5.0, 999.0),
    ('negative', 3.0, -2.0, -5.0, 999.0),
    ('negative', 3.0, -5.0, -2.0, 999.0),
    ('negative', 3.0, 40.0, 5.0, -100.0),                  # a negative capacity
    ('negative zero', -0.0, 4.0, 1.0, 100.0),
    ('negative zero', 3.0, -0.0, 1.0, 100.0),
    ('negative zero', 3.0, 4.0, -0.0, 100.0),
    ('negative zero', -0.0, -0.0, -0.0, 100.0),
    ('negative zero', -0.0, -0.0, 5.0, 100.0),
    ('negative zero', -0.0, 3.0, -0.0, 3.0),               # B == Sm through a negative zero
    ('negative zero', 3.0, -0.0, -0.0, 999.0),             # lake, both zeros of one sign: min(-0, -0), no mixed tie
    ('negative zero', 3.0, -0.0, 5.0, 999.0),
    ('negative zero', 3.0, 5.0, -0.0, 999.0),
    ('negative zero', -0.0, 5.0, 2.0, 999.0),
]

# the same rows under another water-body code: Sm == 250 is now the lake and Sm == 999 is soil
ALT_INDEXING = 250.0
HAND_ALT = [
    ('alt lake', 3.0, 9.0, 5.0, 250.0),
    ('alt lake', 3.0, 5.0, 9.0, 250.0),
    ('alt lake', 3.0, NAN, 9.0, 250.0),
    ('alt lake', 3.0, 5.0, 5.0, 250.0),
    ('alt 999 is soil', 500.0, 9.0, 5.0, 999.0),
    ('alt 999 is soil', 998.0, 9.0, 5.0, 999.0),           # B >= Sm
    ('alt 999 is soil', 0.0, 0.0, 5.0, 999.0),
    ('alt soil', 125.0, 9.0, 5.0, 250.0000000000001),
    ('alt soil', 125.0, 9.0, 5.0, 249.9999999999999),
    ('alt no soil', 3.0, 9.0, 5.0, 0.0),
]


def _pack(rows, grid=None):
    lab = np.array([r[0] for r in rows])
    ch, p, pet, sm = (np.array([r[i] for r in rows], dtype=np.float64) for i in (1, 2, 3, 4))
    if grid is not None:
        lab = np.concatenate([np.full(grid[0].size, 'grid'), lab])
        ch, p, pet, sm = (np.concatenate([g, h]) for g, h in zip(grid, (ch, p, pet, sm)))
    return SimpleNamespace(label=lab, ch=ch, p=p, pet=pet, sm=sm, ncell=ch.size)


def set_a(seed=SEED_A):
    """The grid (2,850 cells) and the hand-written blocks, water-body code 999."""
    rng = np.random.default_rng(seed)
    x, sm, pet, p = np.array(list(itertools.product(X_VALUES, SM_VALUES, PET_VALUES, P_VALUES)), dtype=np.float64).T
    jit = lambda a: a * (1.0 + rng.uniform(-1e-3, 1e-3, a.shape))          # noqa: E731
    x, sm, pet, p = jit(x), jit(sm), jit(pet), jit(p)
    cs = _pack(HAND, (x * sm, p, pet, sm))
    cs.indexing = 999.0
    return cs


def set_a_alt():
    cs = _pack(HAND_ALT)
    cs.indexing = ALT_INDEXING
    return cs


def scale_a(cs):
    """|ch| + |P| + |PET| + Sm per cell (Sm dropped on a water body); a term that is not finite counts 0."""
    f = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)                 # noqa: E731
    s = f(cs.ch) + f(cs.p) + f(cs.pet) + np.where(cs.sm == cs.indexing, 0.0, f(cs.sm))
    return np.where(s > 0, s, 1.0)


NC_B, NM_B = 1200, 50
SM0_FACTORS = (0.0, 0.05, 0.5, 1.0, 1.3, 2.6)
SPINUPS_B = (0, 12, 50)


def set_b(seed=SEED_B):
    rng = np.random.default_rng(seed)
    nc, nm = NC_B, NM_B
    c = np.arange(nc)
    sm = rng.uniform(5, 600, nc)
    sm[13::17] = rng.uniform(0.5, 5, len(sm[13::17]))      # tiny capacity: B >= Sm often
    sm[::29] = 999.0                                       # water bodies
    sm[7::61] = 0.0                                        # no soil
    sm[11::173] = np.nan                                   # missing capacity
    # classes by c mod 5 (below); the factor changes every 5 cells and again every 30, so that the classes made by
    # strides 17, 29 and 61 meet every factor too
    sm0 = sm * np.array(SM0_FACTORS)[(c // 5 + c // 30) % 6]
    pet = rng.uniform(0, 180, (nc, nm))
    precip = rng.gamma(1.2, 50.0, (nc, nm))
    precip[1::5] *= 0.05                                   # dry cells: the 0.1 floor and Sav <= 0
    pet[2::5] *= 3.0                                       # tripled PET
    precip[3::5] *= rng.random((len(precip[3::5]), nm)) < 0.3          # no precipitation in most months
    hole = (c % 35 == 4)                                   # a few missing values, one month per cell
    pet[hole, (c[hole] * 7) % nm] = np.nan
    hole = (c % 35 == 19)
    precip[hole, (c[hole] * 3) % nm] = np.nan
    precip[::58, -1] = np.nan                              # lakes with NaN P in a column the reference driver reads
    return SimpleNamespace(ncell=nc, nmonths=nm, pet=pet, precip=precip, sm=sm, sm0=sm0, indexing=999.0)


def scale_b(cs):
    """max|P| + max|PET| + Sm + |sm0| per cell (Sm dropped on a water body); NaN months and NaN capacities count 0."""
    f = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)                 # noqa: E731
    s = f(cs.precip).max(axis=1) + f(cs.pet).max(axis=1) + np.where(cs.sm == cs.indexing, 0.0, f(cs.sm)) + f(cs.sm0)
    return np.where(s > 0, s, 1.0)


def constant_precip(cs):
    """Set B with every precipitation column equal to the last: `monthly` then reads what `reference` reads."""
    out = SimpleNamespace(**vars(cs))
    out.precip = np.repeat(cs.precip[:, -1:], cs.nmonths, axis=1)
    return out


GOLDEN_B_CELLS = np.arange(3, NC_B, 13)                    # the slice of B whose reference outputs gwam_edges.npz holds
GOLDEN_B_SPINUP = 12

# ---- set C
NMONTHS_C = (2, 14, 16, 18, 30, 34, 50)
NCELL_C = (1, 7, 31, 32, 33, 65, 257)
ROWS_C = (0, 1, 31, 32, 33, 34, 66, 67, 100, 125, 254, 256)            # cell indices one row of B is placed at
TMS = 16                                                   # months per tile of k_gwam_tile


def shifts(ncell, nmonths):
    return (np.arange(ncell) * nmonths) % TMS


def tiles_spanned(shift, nmonths):
    """Tiles of 16 months a row of nmonths touches when it starts at month `shift` of the first tile."""
    return (shift + nmonths - 1) // TMS + 1


def shapes_c():
    return [(nm, nc) for nm in NMONTHS_C for nc in NCELL_C]


def rows_for(cs, ncell, nmonths, first=0):
    """ncell consecutive rows of B from cell `first` (wrapping), cut to nmonths: an [ncell, nmonths] problem."""
    idx = (first + np.arange(ncell)) % cs.ncell
    return SimpleNamespace(ncell=ncell, nmonths=nmonths, pet=np.ascontiguousarray(cs.pet[idx, :nmonths]),
                           precip=np.ascontiguousarray(cs.precip[idx, :nmonths]), sm=cs.sm[idx].copy(),
                           sm0=cs.sm0[idx].copy(), indexing=cs.indexing)


# ---- the long-double truth, the float64 restatement under three exps, and the bar they set (computed once per process)
NEAR = 1e-9                                                # x scale: closer to a discontinuity than this, a cell is left out
BAR_FACTOR = 4.0                                           # the device's bar is BAR_FACTOR x E_host
_cache = {}


def near_discontinuity(gap, scale):
    """An exact tie (gap 0) is structural: it is exact in the inputs and falls on one side in every precision."""
    return (gap != 0) & (gap < NEAR * scale)


def _truth_a(alt):
    import gwam_np as G
    cs = set_a_alt() if alt else set_a()
    t = G.month(cs.pet, cs.p, cs.sm, cs.ch, G.LD, None, cs.indexing)
    hosts = [G.month(cs.pet, cs.p, cs.sm, cs.ch, np.float64, G.exp_ulp(k), cs.indexing) for k in (0, 1, -1)]
    scale = scale_a(cs)
    left = near_discontinuity(t[3].gap_b, scale) | near_discontinuity(t[3].gap_8, scale)
    e = max(G.worst_error(h[i], t[i], scale, ~left) for h in hosts for i in range(3))
    return SimpleNamespace(cs=cs, truth=t[:3], rec=t[3], hosts=hosts, scale=scale, left_out=left, e_host=e)


def truth_a(alt=False):
    """Set A in long double: .truth (aet, q, sav), .rec, .hosts (the float64 restatement with exp moved 0, +1, -1 ulp),
    .scale, .left_out, .e_host, .bar.  ``alt`` gives the rows under the other water-body code; they are part of set A, and
    E_host and the bar are those of the whole set."""
    if 'a' not in _cache:
        both = {k: _truth_a(k) for k in (False, True)}
        for t in both.values():
            t.e_host = max(x.e_host for x in both.values())
            t.bar = BAR_FACTOR * t.e_host
        _cache['a'] = both
    return _cache['a'][alt]


def truth_b(monthly, spinup, constant=False):
    """Set B marched in long double; fields as truth_a, .truth = (aet, q, sav, sm_end)."""
    import gwam_np as G
    key = ('b', monthly, spinup, constant)
    if key not in _cache:
        cs = constant_precip(set_b()) if constant else set_b()
        run = lambda T, f: G.series(cs.pet, cs.precip, cs.sm, cs.sm0, spinup, monthly, T, f, cs.indexing)      # noqa: E731
        t = run(G.LD, None)
        hosts = [run(np.float64, G.exp_ulp(k)) for k in (0, 1, -1)]
        scale = scale_b(cs)
        left = near_discontinuity(t[3].near_b, scale) | near_discontinuity(t[3].near_8, scale)
        four = lambda r: (r[0], r[1], r[2], r[3].sm_end)                                                         # noqa: E731
        e = max(G.worst_error(x, y, scale, ~left) for h in hosts for x, y in zip(four(h), four(t)))
        _cache[key] = SimpleNamespace(cs=cs, truth=four(t), rec=t[3], hosts=[four(h) for h in hosts], scale=scale,
                                      left_out=left, e_host=e, bar=BAR_FACTOR * e)
    return _cache[key]
