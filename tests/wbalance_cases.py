"""The rows the water balance tests share (tests/test_wbalance_host.py, tests/test_gpu_wbalance.py, the golden values of
tests/golden/make_golden_wbalance.py): one quadruple (P, PET, Q, AET) of every kind at every year count, from fixed seeds.  Every
batch is run with its AET and without (`aet=None`): the kind `no_aet` has gaps in AET only, so the two runs include different
months."""
import numpy as np

# years: 1, 2, 3 the guards (one year, fewer than 3 for the least squares); 5; 21 / 22 under and just over one pass of the 256
# lanes over the months (252 / 264 columns); 33 and 64 / 65 on both sides of two powers of two of the sort (32, 64); 257 over one
# pass of Y256; 341 the limit (4092 columns)
YEARS = (1, 2, 3, 5, 21, 22, 33, 64, 65, 257, 341)
KINDS = ('humid', 'arid', 'equal', 'q_zero', 'q_over_p', 'p_const', 'collinear', 'ties', 'lagged', 'scattered', 'year_nan',
         'all_nan', 'no_aet', 'shifted', 'signed_zeros')
MAX_LAG = 6
OMEGA0 = 2.6


def quadruple(kind, nyear):
    ncol = 12 * nyear
    rng = np.random.default_rng(9100 + 131 * KINDS.index(kind) + nyear)
    t = np.arange(ncol)
    season = 1.0 + 0.6 * np.sin(2.0 * np.pi * (t % 12) / 12.0)
    wet = np.repeat(rng.gamma(8.0, 1.0 / 8.0, nyear), 12)                       # wet and dry years
    p = np.round(80.0 * wet * season * rng.gamma(4.0, 0.25, ncol), 6)
    pet = np.round(55.0 * (2.0 - season) * np.repeat(rng.normal(1.0, 0.05, nyear), 12) * rng.uniform(0.9, 1.1, ncol), 6)
    if kind == 'arid':
        pet = np.round(pet * 3.5, 6)
    aet = np.round(np.minimum(p, pet) * rng.uniform(0.7, 0.95, ncol), 6)
    q = np.round((p - aet) * rng.uniform(0.8, 1.1, ncol), 6)
    if kind == 'equal':                 # whole numbers: every sum is exact in any order, so petbar == pbar exactly
        p = np.round(p, 0)
        pet = p.reshape(nyear, 12)[:, ::-1].reshape(ncol).copy()
        aet, q = np.round(0.6 * p, 6), np.round(0.4 * p, 6)
    elif kind == 'q_zero':
        q = np.zeros(ncol)
    elif kind == 'q_over_p':
        q = np.round(1.3 * p, 6)
    elif kind == 'p_const':             # the same whole numbers every year: dP_y = 0 exactly
        p = np.tile(np.round(p[:12], 0), nyear)
    elif kind == 'collinear':           # PET = 2 P exactly, in every sum too
        pet = 2.0 * p
    elif kind == 'ties':                # a few year patterns of whole numbers, Q an exact fraction of P: many equal e_y
        pattern = np.round(rng.uniform(20.0, 200.0, (3, 12)), 0)
        which = rng.integers(0, 3, nyear)
        p = pattern[which].reshape(ncol)
        q = (p.reshape(nyear, 12) * np.array([0.5, 0.5, 0.25])[which][:, None]).reshape(ncol)
    elif kind == 'lagged':              # Q_t = P_{t-3} on a P without seasons
        p = np.round(rng.gamma(2.0, 40.0, ncol), 6)
        q = np.concatenate([p[:3][::-1], p[:-3]])
    elif kind == 'scattered':           # in Q only
        hit = rng.random(ncol)
        q = np.where(hit < 0.06, np.nan, np.where(hit < 0.09, np.inf, np.where(hit < 0.12, -np.inf, q)))
    elif kind == 'year_nan':
        y = nyear // 2
        p[12 * y:12 * y + 12] = np.nan
    elif kind == 'all_nan':
        p, pet, q, aet = (np.full(ncol, np.nan) for _ in range(4))
    elif kind == 'no_aet':              # gaps in AET only
        aet = np.where(rng.random(ncol) < 0.05, np.nan, aet)
    elif kind == 'shifted':
        p, pet, q, aet = p + 1.0e6, pet + 1.0e6, q + 1.0e6, aet + 1.0e6
    elif kind == 'signed_zeros':
        p = np.where(rng.random(ncol) < 0.3, -0.0, np.where(rng.random(ncol) < 0.2, 0.0, p))
        q = np.where(p == 0.0, -0.0, q)
        aet = np.where(p == 0.0, 0.0, aet)
    return tuple(np.ascontiguousarray(v, dtype=np.float64) for v in (p, pet, q, aet))


def rows(nyear):
    """(P, PET, Q, AET), each [len(KINDS), 12 nyear]: one quadruple of every kind."""
    quads = [quadruple(kind, nyear) for kind in KINDS]
    return tuple(np.stack([quad[v] for quad in quads]) for v in range(4))
