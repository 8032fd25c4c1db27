"""GPU tests of the three simple PET stages -- k_hargreaves_pet (csrc/xh_gwam.hip), k_hs_pet, k_trn_daylight and k_trn_pet
(csrc/xh_pet_ext.hip) -- at every branch and edge, through the C ABI, against a long-double numpy truth (tests/pet_np.py) on
the case sets of tests/pet_cases.py.  tests/test_gpu_hgm.py and tests/test_gpu_pet_ext.py stay as they are.

The bar is not a literal: tests/pet_cases.py computes E_host, the worst |float64 restatement - long-double truth| / scale of
a correct float64 evaluation (numpy's functions, and each transcendental moved one ulp either way), and the device is held to
4 x E_host per set.  The scale is per element (pet_np): it carries the first-order sensitivity to the sunset argument, which
Hargreaves-Samani needs (PET jumps from its maximum to 0 at tn = -1, where the reference sets acs = 0 instead of pi) and the
daylight table needs next to a clipped day.  Bits are asserted only where no transcendental decides an output, and between
device runs: numpy sums a year's heat index and a month's days with eight accumulators, the device one after the other, so
a float64 restatement and the device differ in the last bits of about half of all rows.

Measured on an MI355X (printed by test_within_bar; errors in units of scale, E_host also in ulp = 2^-53 of scale).  No case is
left out of any bar, no branch differs between float64 and long double, and no defect was found in the kernels or wrappers.

    stage, set                                   E_host              bar = 4 E_host   device error   error / bar
    Hargreaves   A (306 cells x 36 months)       7.30e-16  6.6 ulp   2.92e-15         5.27e-16       0.180
    Hargreaves   B (181 x 24)                    7.08e-16  6.4 ulp   2.83e-15         5.31e-16       0.187
    HS           A (204 cells x 48 months)       4.18e-16  3.8 ulp   1.67e-15         2.45e-16       0.146
    HS           B (181 x 24)                    5.92e-16  5.3 ulp   2.37e-15         4.28e-16       0.181
    daylight     A (30 x 24)                     2.65e-16  2.4 ulp   1.06e-15         2.42e-16       0.228
    daylight     B (181 x 24)                    3.08e-16  2.8 ulp   1.23e-15         2.68e-16       0.217
    Thornthwaite A (72 cells x 12, 6 years)      1.64e-16  1.5 ulp   6.58e-16         1.15e-16       0.175
    Thornthwaite B (300 x 12..156, 2 orders)     3.92e-16  3.5 ulp   1.57e-15         2.62e-16       0.167

Every output sits inside a sentinel-guarded allocation; nothing outside it may be written, nothing inside left unwritten.
The 64-bit quotient path of the two element kernels (n > 2^32) needs 34 GB per array and stays untested.

Mutation check (not committed; one thing changed at a time in a scratch build of the library, loaded through XH_LIBRARY, this
file run against each; every mutant keeps all indices inside its arrays):

    tn < -1.0 -> tn <= -1.0 (HS)          none, and no portable input can: the two differ only at tn == -1.0 exactly, where tn is
                                          the rounded product of the host's tan(delta) and the device's tan(phi); whether some
                                          latitude makes it exactly -1 depends on the last bit of both.  Set A stands 1e-6 off
    t < 0.0 -> t <= 0.0 (HS)              test_within_bar[hs-a], test_exact_hs (tas = -0.0 and 0 give 0 instead of the formula)
    arg < -1.0 ? pi : 0 swapped           test_within_bar[hg-a], [hg-b], test_exact_hargreaves
    D < 0 dropped                         test_within_bar[hg-a], [hg-b], test_exact_hargreaves, test_grid_stride[hg] (NaN from sqrt)
    yr % 100 != 0 dropped                 test_within_bar[tr-a], [tr-b], test_exact_thornthwaite_and_leap_years,
                                          test_thornthwaite_group_edges[51-5], ..._prefix_and_reference_columns[5, 7, 12, 13]
    yr % 400 == 0 dropped                 test_within_bar[tr-a], test_exact_thornthwaite_and_leap_years
    (12 y + k) / nyears -> k              test_within_bar[tr-b], test_thornthwaite_group_edges[51-5, 64-4, 171-3],
                                          ..._prefix_and_reference_columns[2, 3, 5, 7, 12, 13]
    I != 0.0 dropped                      test_within_bar[tr-a], test_exact_thornthwaite_and_leap_years (NaN where I = 0)
    d0 one day late (index capped at 365) test_within_bar[dl-a], [dl-b], [tr-a], [tr-b], test_exact_daylight[a], [b],
                                          test_thornthwaite_group_edges (all five)
    TLD 13 -> 12 (allocation kept)        21 tests: every Thornthwaite test but the daylight table's
"""
import numpy as np
import pytest

import pet_cases as C
import pet_np as P

pytestmark = pytest.mark.gpu

GUARD = 16                                                 # doubles before and after every output allocation
SENTINEL = np.uint64(0x7ff8dead0000beef)                   # a NaN no arithmetic makes
ULP = 2.0 ** -53
NCELLS = (1, 21, 22, 255, 256, 257)


def _ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


class Guarded:
    """An output of n doubles inside a larger allocation filled with a sentinel."""

    def __init__(self, ctx, shape, guard=GUARD):
        self.shape, self.n, self.guard = shape, int(np.prod(shape)), guard
        self.buf = ctx.upload(np.full(self.n + 2 * guard, SENTINEL, dtype=np.uint64).view(np.float64))
        self.ptr = self.buf.ptr + 8 * guard

    def take(self, name):
        raw = self.buf.download()
        self.buf.free()
        edge = np.concatenate([raw[:self.guard], raw[self.guard + self.n:]]).view(np.uint64)
        assert (edge == SENTINEL).all(), name + ': written outside the array'
        body = raw[self.guard:self.guard + self.n]
        assert not (body.view(np.uint64) == SENTINEL).any(), name + ': elements left unwritten'
        return body.reshape(self.shape).copy()


def run_hg(temp, dtr, lat, dec, dr, nd):
    ctx = _ctx()
    temp = np.ascontiguousarray(temp, dtype=np.float64)
    nc, nm = temp.shape
    ins = [ctx.upload(temp), ctx.upload(np.ascontiguousarray(dtr, dtype=np.float64)), ctx.upload(np.asarray(lat, dtype=np.float64))]
    out = Guarded(ctx, (nc, nm))
    try:
        ctx.hargreaves_pet(nc, nm, ins[0], ins[1], ins[2], dec[:nm], dr[:nm], nd[:nm], out.ptr)
        ctx.sync()
    finally:
        for b in ins:
            b.free()
    return out.take('hargreaves')


def run_hs(tas, tmax, tmin, lat, nd):
    ctx = _ctx()
    tas = np.ascontiguousarray(tas, dtype=np.float64)
    nc, nm = tas.shape
    ins = [ctx.upload(np.ascontiguousarray(a, dtype=np.float64)) for a in (tas, tmax, tmin, lat)]
    out = Guarded(ctx, (nc, nm))
    try:
        ctx.hs_pet(nc, nm, ins[0], ins[1], ins[2], ins[3], nd[:nm], out.ptr)
        ctx.sync()
    finally:
        for b in ins:
            b.free()
    return out.take('hs')


def run_tr(tas, lat, y0, monthly=False, table=True):
    """(PET or None, the [ncell, 24] daylight table or None).  tas = None: nmonths = 0, daylight only."""
    from xanthos_amd import _hip
    ctx = _ctx()
    lat = np.asarray(lat, dtype=np.float64)
    nc, nm = lat.size, (0 if tas is None else tas.shape[1])
    ins = [ctx.upload(lat)] + ([ctx.upload(np.ascontiguousarray(tas, dtype=np.float64))] if nm else [])
    pet = Guarded(ctx, (nc, nm)) if nm else None
    dl = Guarded(ctx, (nc, 24)) if table else None
    try:
        ctx.thornthwaite_pet(nc, nm, y0, _hip.XH_DAYLIGHT_MONTHLY if monthly else _hip.XH_DAYLIGHT_REFERENCE,
                             ins[1] if nm else None, ins[0], pet.ptr if nm else None, dl.ptr if table else None)
        ctx.sync()
    finally:
        for b in ins:
            b.free()
    return (pet.take('thornthwaite') if nm else None), (dl.take('daylight') if table else None)


_runs = {}


def device(stage, which, *key):
    """The device's output of one run of a set (computed once per process)."""
    k = (stage, which) + key
    if k not in _runs:
        cs = C.truth(stage, which, *key).cs
        if stage == 'hg':
            _runs[k] = run_hg(cs.temp, cs.dtr, cs.lat, cs.dec, cs.dr, cs.nd)
        elif stage == 'hs':
            _runs[k] = run_hs(cs.tas, cs.tmax, cs.tmin, cs.lat, cs.nd)
        elif stage == 'dl':
            _runs[k] = run_tr(None, cs.lat, 1970)[1]
        elif which == 'a':
            _runs[k] = run_tr(cs.tas, cs.lat, key[0])[0]
        else:
            _runs[k] = run_tr(cs.tas, cs.lat, C.Y0_B, monthly=key[1])[0]
    return _runs[k]


# ------------------------------------------------------------------------------------------- 1. within the bar of the truth
@pytest.mark.parametrize('stage,which', [(s, w) for s in ('hg', 'hs', 'dl', 'tr') for w in ('a', 'b')])
def test_within_bar(stage, which):
    bar, worst = C.bar(stage, which), 0.0
    for key in C.runs(stage, which):
        t, x = C.truth(stage, which, *key), device(stage, which, *key)
        assert not t.left_out.any()
        assert P.classes_equal(x, t.host), 'NaN, inf or zero mask differs from the float64 restatement {}'.format(key)
        e = C.worst(x, t)
        worst = max(worst, e)
        print('{} {} {}: error {:.3e} x scale'.format(stage, which, key, e))
    print('{} {}: E_host {:.3e} ({:.1f} ulp), bar {:.3e}, device error {:.3e}, ratio {:.3f}'.format(
        stage, which, bar / 4, bar / 4 / ULP, bar, worst, worst / bar))
    assert worst <= bar


# ------------------------------------------------------------------------------------------- 2. exact outputs
def test_exact_hargreaves():
    t, x = C.truth('hg', 'a'), device('hg', 'a')
    b, cs = t.rec.branch, t.cs
    zero = t.host == 0
    assert zero.sum() > 2000 and P.same(x[zero], t.host[zero])
    night = ((b & P.HG_MASK) == P.HG_ABOVE) & ~np.isnan(cs.lat)[:, None]              # ws = 0: no insolation at all
    assert night.sum() > 500 and (x[night] == 0).all()
    # D < 0 -> 0 and sqrt(0) = 0 (an infinite T, DBL_MAX after nan_to_num, overflows first and gives inf x 0)
    neg = ((b & P.HG_NEG_D) != 0) & ~np.isnan(cs.lat)[:, None] & ~np.isinf(cs.temp)
    assert neg.sum() > 1000 and (x[neg] == 0).all()
    clipped = (b & P.HG_NEG_EVAP) != 0                                                 # evap < 0 -> 0
    assert clipped.sum() > 300 and (x[clipped] == 0).all()
    nan_t = np.isnan(cs.temp) & (cs.dtr == 12.0) & ((b & P.HG_MASK) == P.HG_BELOW)    # a NaN temperature counts as 0 degrees
    assert nan_t.any() and (x[nan_t] > 0).all()


def test_exact_hs():
    t, x = C.truth('hs', 'a'), device('hs', 'a')
    b, cs = t.rec.branch, t.cs
    cold = b == P.HS_COLD
    assert cold.sum() > 1000 and P.same_bits(x[cold], np.zeros(int(cold.sum())))       # +0, whatever the other inputs
    assert np.isnan(cs.tmax[cold]).any() and np.isnan(cs.lat[np.nonzero(cold)[0]]).any()
    for v in (-0.0, 0.0, 5e-324):                                                      # not < 0: the formula, at t + 17.8 = 17.8
        m = _is(cs.tas, v) & (b == P.HS_IN) & ((cs.ordering == 0) | (cs.ordering == 2))
        assert m.sum() > 50 and (x[m] > 0).all(), v
    for v in (-5e-324, -1.0):
        assert P.same_bits(x[_is(cs.tas, v)], np.zeros(int(_is(cs.tas, v).sum()))), v
    lat_ok = ~np.isnan(cs.lat)[:, None]
    assert np.isnan(x[np.isnan(cs.tas)]).all()                                         # a NaN tas is not < 0 and gives NaN
    out = ((b == P.HS_BELOW) | (b == P.HS_ABOVE)) & np.isfinite(cs.tas) & (cs.ordering < 3) & lat_ok
    assert out.sum() > 1000 and P.same_bits(x[out], np.zeros(int(out.sum())))          # acs = 0 on BOTH sides: ra = 0
    zero = t.host == 0
    assert P.same(x[zero], t.host[zero])
    # month m of the call takes the declination of month m % 12 and the days of month m
    again = run_hs(cs.tas[:, 12:24], cs.tmax[:, 12:24], cs.tmin[:, 12:24], cs.lat, cs.nd[12:24])
    assert P.same_bits(again, x[:, 12:24])


def _is(a, v):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.isnan(a) if v != v else a.view(np.uint64) == np.float64(v).view(np.uint64)


@pytest.mark.parametrize('which', ['a', 'b'])
def test_exact_daylight(which):
    t, x = C.truth('dl', which), device('dl', which)
    days = np.array(P.MONTHDAYS + P.LEAP_MONTHDAYS)
    lo, hi = t.rec.lo, t.rec.hi
    assert (hi == days).any() and P.same_bits(x[hi == days], np.zeros(int((hi == days).sum())))          # polar night: 0 h
    assert (lo == days).any() and P.same_bits(x[lo == days], np.full(int((lo == days).sum()), 24.0))     # polar day: 24 h
    full = lo + hi == days                                  # every day clipped: multiples of 24 / days, no acos in them
    assert P.same_bits(x[full], t.host[full])
    lat = t.cs.lat
    north, south = x[lat == np.pi / 2], x[lat == -np.pi / 2]
    assert north.shape == (1, 24) and south.shape == (1, 24) and P.same_bits(24 - north, south)
    assert (x[lat == 0] == 12).all()


def test_exact_thornthwaite_and_leap_years():
    a = C.cases('tr', 'a')
    lab = a.label
    ok = ~np.isnan(a.lat)
    runs = {y: device('tr', 'a', y) for y in C.YEARS_A}
    for y, x in runs.items():
        t = C.truth('tr', 'a', y)
        for name in ('all negative', 'all NaN'):                                       # I == 0 -> 0; NaN counts as 0
            m = (lab == name) & ok
            assert P.same_bits(x[m], np.zeros((int(m.sum()), 12))), (y, name)
        zero = ((t.rec.branch & 3) != P.TR_WARM) & ok[:, None]                         # t < 0, t = +-0, NaN: +0
        assert zero.sum() > 200 and P.same_bits(x[zero], np.zeros(int(zero.sum())))
        assert np.isnan(x[lab == 'inf month']).all()
    # the leap table and 29 days are used exactly in 1896, 1904, 2000 and 2400
    for y in (1904, 2000, 2400):
        assert P.same_bits(runs[y], runs[1896]), y
    assert P.same_bits(runs[2100], runs[1900])
    _, dl = run_tr(None, a.lat, 1970)
    m = (lab == 'ordinary') & ok & (np.abs(a.lat) < 1.0)
    leap, common = runs[1896][m], runs[1900][m]
    # PET = pu (L / 12) (N / 30) with the same pu: the quotient is that of L[12 + k] N_leap and L[k] N_common, to the ten
    # roundings of the two PET, their quotient and the expectation, each at most 2^-53
    want = (dl[m, 12:] / dl[m, :12]) * (np.array(P.LEAP_MONTHDAYS) / np.array(P.MONTHDAYS))
    assert m.sum() == 3 and np.abs(leap / common / want - 1).max() < 16 * ULP
    assert (np.abs(leap[:, 1] / common[:, 1] - 29 / 28) < 0.02).all() and (leap[:, 1] != common[:, 1]).all()


# ------------------------------------------------------------------------------------------- 3. invariance in bits
def _rows(n, total, first):
    return (first + np.arange(n)) % total


@pytest.mark.parametrize('ncell', NCELLS)
def test_element_kernels_any_ncell_any_index_any_prefix(ncell):
    """ncell rows of set B, at other cell indices than in the grid and cut to a prefix of the months: the bits of the grid."""
    for k, nm in enumerate((24, 7, 13)):
        idx = _rows(ncell, 181, 17 * ncell + 50 * k)
        cs, big = C.cases('hg', 'b'), device('hg', 'b')
        assert P.same_bits(run_hg(cs.temp[idx, :nm], cs.dtr[idx, :nm], cs.lat[idx], cs.dec, cs.dr, cs.nd), big[idx, :nm])
        cs, big = C.cases('hs', 'b'), device('hs', 'b')
        assert P.same_bits(run_hs(cs.tas[idx, :nm], cs.tmax[idx, :nm], cs.tmin[idx, :nm], cs.lat[idx], cs.nd), big[idx, :nm])
    cs, big = C.cases('dl', 'b'), device('dl', 'b')
    idx = _rows(ncell, 181, 17 * ncell)
    assert P.same_bits(run_tr(None, cs.lat[idx], 2001)[1], big[idx])


@pytest.mark.parametrize('ncell', NCELLS)
def test_thornthwaite_any_ncell_any_index(ncell):
    """Rows of set B at other cell indices, in a launch of ncell cells: the bits of the 300-cell run, with and without
    d_daylight, and the table of an nmonths = 0 call is the table of the run."""
    ny = 3
    cs = C.cases('tr', 'b', ny)
    idx = _rows(ncell, C.NC_TR_B, 41 * ncell)
    for monthly in (False, True):
        big = device('tr', 'b', ny, monthly)
        pet, dl = run_tr(cs.tas[idx], cs.lat[idx], C.Y0_B, monthly)
        assert P.same_bits(pet, big[idx])
        assert P.same_bits(run_tr(cs.tas[idx], cs.lat[idx], C.Y0_B, monthly, table=False)[0], pet)
        assert P.same_bits(run_tr(None, cs.lat[idx], C.Y0_B)[1], dl)


@pytest.mark.parametrize('ncell,ny', [(1, 1), (51, 5), (64, 4), (257, 1), (171, 3)])
def test_thornthwaite_group_edges(ncell, ny):
    """ncell x nyears = 1, 255, 256, 257 and 513 (cell, year) groups -- a last block of 1, 255, 256 (none short) and 1 --
    against the same rows in a 300-cell launch, whose blocks cut the groups elsewhere; and against the truth."""
    b = C.cases('tr', 'b')
    tas, lat = b.tas[:, :12 * ny], b.lat
    idx = _rows(ncell, C.NC_TR_B, 7)
    for monthly in (False, True):
        big = run_tr(tas, lat, C.Y0_B, monthly)[0]
        assert P.same_bits(run_tr(tas[idx], lat[idx], C.Y0_B, monthly)[0], big[idx]), (ncell, ny, monthly)
        t = C.truth('tr', 'b', ny, monthly)
        assert P.classes_equal(big, t.host) and C.worst(big, t) <= C.bar('tr', 'b')


@pytest.mark.parametrize('ny', C.NYEARS_B)
def test_thornthwaite_prefix_and_reference_columns(ny):
    """`monthly`: a year's PET does not depend on how many years follow it.  `reference`: the leap years, and the months
    whose predicted column (12 y + k) // nyears is k, have the bits of `monthly`; every other month is `monthly` x
    L[column] / L[k] to the ten roundings of the two PET, their quotient and the expectation."""
    cs = C.cases('tr', 'b', ny)
    mon, ref = device('tr', 'b', ny, True), device('tr', 'b', ny, False)
    assert P.same_bits(mon, device('tr', 'b', 13, True)[:, :12 * ny])
    cols = C.truth('tr', 'b', ny, False).rec.cols
    mcols = C.truth('tr', 'b', ny, True).rec.cols
    same = cols == mcols
    assert P.same_bits(ref[:, same], mon[:, same])
    if ny > 1:
        assert not same.all()
        dl = run_tr(None, cs.lat, C.Y0_B)[1]
        with np.errstate(all='ignore'):
            want = mon[:, ~same] * (dl[:, cols[~same]] / dl[:, mcols[~same]])
            got = ref[:, ~same]
            ok = np.isfinite(want) & (want != 0) & np.isfinite(got)
            assert ok.mean() > 0.3 and (np.abs(got[ok] / want[ok] - 1) < 16 * ULP).all()
            moved = ok & (np.abs(dl[:, cols[~same]] / dl[:, mcols[~same]] - 1) > 1e-6)
        assert moved.any() and (got[moved] != mon[:, ~same][moved]).all()


@pytest.mark.parametrize('stage', ['hg', 'hs'])
def test_grid_stride(stage):
    """n just above multiProcessorCount x 32 x 256, the cap of the element kernels' grid: some lanes take a second element.
    The bits of the same rows run 400 cells at a time (one element per lane)."""
    cu = _ctx().cu_count()
    nm = 480
    nc = (cu * 32 * 256) // nm + 30
    assert cu * 32 * 256 < nc * nm < cu * 32 * 256 + 32 * nm
    rng = np.random.default_rng(C.SEED + 5)
    lat = rng.uniform(-90, 90, nc)
    t = rng.uniform(-30, 40, (nc, nm))
    d = rng.uniform(-2, 20, (nc, nm))
    if stage == 'hg':
        dec, dr, nd = C.month_factors(1861, 1900)
        f = lambda r: run_hg(t[r], d[r], np.radians(lat[r]), dec, dr, nd)                # noqa: E731
    else:
        nd = C.days(range(1861, 1901))
        f = lambda r: run_hs(t[r], t[r] + d[r], t[r] - 3, lat[r], nd)                    # noqa: E731
    whole = f(slice(None))
    assert np.isfinite(whole).all() and (whole > 0).mean() > 0.3
    for i in range(0, nc, 400):
        r = slice(i, min(i + 400, nc))
        assert P.same_bits(f(r), whole[r]), 'cells {}..'.format(i)
