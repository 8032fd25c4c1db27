"""CPU tests of the apparatus that tests/test_gpu_pet_edges.py holds the three simple PET stages to (tests/pet_np.py,
tests/pet_cases.py): that the case sets reach every branch on both sides of every comparison, that the numpy restatements
are the reference's modules (tests/golden/pet_edges.npz), that no case sits on a discontinuity and no branch differs between
float64 and long double, and what error a correct float64 evaluation has against the long-double truth -- E_host, a quarter
of the device's bar.  No GPU, no reference tree.

E_host here, in ulp (2^-53) of scale (printed by test_bar); GWAM's worst accepted figure is 32.8:

    Hargreaves  A 6.6  B 6.4      Hargreaves-Samani  A 3.8  B 5.3      daylight  A 2.4  B 2.8      Thornthwaite  A 1.5  B 3.5

The daylight scale is not 24 h alone.  With 24 h, set A came out at 91.7 ulp: a day whose argument x lies 1e-7 inside +-1 has
d acos / dx = 1 / sqrt(1 - x^2) = 2,200, and the tangent of a latitude near a pole amplifies its own rounding.  The term
(24 / pi) x mean over the month's unclipped days of |x| c_phi / sqrt(1 - x^2) is added to the scale (pet_np.daylight), and
Thornthwaite's scale carries the daylight's.
"""
import numpy as np
import pytest

import pet_cases as C
import pet_np as P

ULP = 2.0 ** -53
GWAM_WORST = 32.8 * ULP
SETS = [(s, w) for s in ('hg', 'hs', 'dl', 'tr') for w in ('a', 'b')]


def test_long_double_is_extended():
    assert np.finfo(P.LD).nmant >= 63


# ------------------------------------------------------------------------------------------- coverage
def _sides(t, col_of, inside, below, above, branch_of=lambda b: b, skip=None):
    """Every latitude solved for `<unit> k arg <target>` takes, in its unit (month, day) k, the branch its label names,
    with a gap of the margin."""
    lab = t.cs.label
    seen = 0
    for i in np.nonzero(np.char.find(lab, ' arg ') >= 0)[0]:
        unit, target = lab[i].split(' arg ')
        k = int(unit.split()[1])
        sign, m = (1 if target[0] == '+' else -1), float(target[3:])
        inner = target[2] == '-'
        want = inside if inner else (above if sign > 0 else below)
        for col in col_of(k):
            if t.rec.branch[i, col] == skip:
                continue
            assert branch_of(t.rec.branch[i, col]) == want, lab[i]
            assert abs(float(np.asarray(t.rec.gap)[i, col]) / m - 1) < 1e-3, lab[i]
            seen += 1
    return seen


def test_coverage_hargreaves():
    t = C.truth('hg', 'a')
    b = t.rec.branch
    assert set(np.unique(b & P.HG_MASK).tolist()) == {P.HG_IN, P.HG_BELOW, P.HG_ABOVE, P.HG_NAN}
    for flag in (P.HG_NEG_D, P.HG_NEG_EVAP):
        for kind in (P.HG_IN, P.HG_BELOW):                 # (above 1 the insolation is 0 and evap is never < 0)
            m = (b & P.HG_MASK) == kind
            assert (b[m] & flag).any() and not (b[m] & flag).all(), (flag, kind)
    # months 0-11 of the table are those the latitudes were solved for; the table repeats with the year's length
    n = _sides(t, lambda k: [k], P.HG_IN, P.HG_BELOW, P.HG_ABOVE, lambda x: x & P.HG_MASK)
    assert n == 3 * 12 * 8
    # every T and every D meets the inside, the polar day and the polar night
    cs = t.cs
    for kind in (P.HG_IN, P.HG_BELOW, P.HG_ABOVE):
        m = (b & P.HG_MASK) == kind
        for v in C.T_VALUES:
            assert np.any(_is(cs.temp[m], v)), (kind, v)
        for v in C.D_VALUES:
            assert np.any(_is(cs.dtr[m], v)), (kind, v)
    assert {'lat 0', 'pole N', 'pole S', 'pole N inside', 'pole S inside', 'lat NaN'} <= set(cs.label.tolist())
    assert (b[cs.label == 'lat NaN'] & P.HG_MASK == P.HG_NAN).all()
    grid = C.truth('hg', 'b').rec.branch
    assert set(np.unique(grid & P.HG_MASK).tolist()) == {P.HG_IN, P.HG_BELOW, P.HG_ABOVE}
    assert (grid & P.HG_NEG_D).any() and (grid & P.HG_NEG_EVAP).any()


def _is(a, v):
    """Elements of a that are v in bits (a NaN is any NaN)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.isnan(a) if v != v else a.view(np.uint64) == np.float64(v).view(np.uint64)


def test_coverage_hs():
    t = C.truth('hs', 'a')
    b, cs = t.rec.branch, t.cs
    assert set(np.unique(b).tolist()) == {P.HS_COLD, P.HS_IN, P.HS_BELOW, P.HS_ABOVE, P.HS_NAN}
    # months k, k + 12, k + 24, k + 36 of the call are month k of the year (m % 12)
    n = _sides(t, lambda k: [k, k + 12, k + 24, k + 36], P.HS_IN, P.HS_BELOW, P.HS_ABOVE, skip=P.HS_COLD)
    assert n > 12 * 8 * 4                                   # all of the cells with tas = 30; the walking cells are cold in places
    for v in C.TAS_VALUES:
        assert np.any(_is(cs.tas, v))
        cold = b[_is(cs.tas, v)] == P.HS_COLD
        assert cold.all() if v < 0 else not cold.any(), v   # -0.0 and NaN are not < 0
    for o in range(len(C.ORDERINGS)):
        for kind in (P.HS_IN, P.HS_BELOW, P.HS_ABOVE):
            assert ((cs.ordering == o) & (b == kind)).any(), (o, kind)
    assert cs.nd.size == 48 and cs.nd[1] == 28 and cs.nd[13] == 28 and cs.nd[37] == 29           # 1900 is common, 2000 leap
    grid = C.truth('hs', 'b').rec.branch
    assert set(np.unique(grid).tolist()) == {P.HS_COLD, P.HS_IN, P.HS_BELOW, P.HS_ABOVE}


def test_coverage_daylight():
    t = C.truth('dl', 'a')
    lat = t.cs.lat
    for leap in (False, True):
        _, r = P.daylight(lat, leap, P.LD)
        x = r.x
        for i in np.nonzero(np.char.find(t.cs.label, ' arg ') >= 0)[0]:
            unit, target = t.cs.label[i].split(' arg ')
            d = int(unit.split()[1]) - 1
            sign, m, inner = (1 if target[0] == '+' else -1), float(target[3:]), target[2] == '-'
            assert (abs(x[i, d]) < 1) == inner and np.sign(x[i, d]) == sign
            assert abs(float(abs(1 - abs(x[i, d]))) / m - 1) < 1e-3
        assert (r.lo > 0).any() and (r.hi > 0).any() and ((r.lo == 0) & (r.hi == 0)).any()
        # whole months of day and of night, and months that are partly clipped
        days = np.array(P.LEAP_MONTHDAYS if leap else P.MONTHDAYS)
        assert (r.lo == days).any() and (r.hi == days).any() and ((r.lo > 0) & (r.lo < days)).any()
    assert (t.rec.branch[np.isnan(lat)] == -1).all()
    g = C.truth('dl', 'b').rec
    assert (g.lo > 0).any() and (g.hi > 0).any()


def test_coverage_thornthwaite():
    want = {1896: True, 1900: False, 1904: True, 2000: True, 2100: False, 2400: True}
    for y in C.YEARS_A:
        t = C.truth('tr', 'a', y)
        b = t.rec.branch
        assert bool((b & P.TR_LEAP).all()) == want[y] and bool((b & P.TR_LEAP).any()) == want[y]
        assert set(np.unique(b & 3).tolist()) == {P.TR_ZERO_I, P.TR_ZERO_T, P.TR_WARM}
        lab = t.cs.label
        for name in ('all negative', 'all NaN'):
            assert (b[lab == name] & 3 == P.TR_ZERO_I).all() and (t.rec.I[lab == name] == 0).all()
        assert ((b[lab == 'one warm among cold'] & 3) == P.TR_WARM).sum(axis=1).tolist() == [1] * len(C.TR_LATS_A)
        assert ((b[lab == 'one zero among warm'] & 3) == P.TR_ZERO_T).sum(axis=1).tolist() == [1] * len(C.TR_LATS_A)
        assert (t.rec.a[lab == '40 throughout'] > 8).all()
    assert [p[0] for p in C.TR_PATTERNS].count('denormal month') == 1 and 5e-324 in dict(C.TR_PATTERNS)['denormal month']
    # set B from 1896: leap and common years, and in reference order every column 0-11 of the common table
    cols = set()
    for ny in C.NYEARS_B:
        t = C.truth('tr', 'b', ny, False)
        leap = [P.isleap(C.Y0_B + y) for y in range(ny)]
        assert leap[0] and (ny < 5 or not leap[4]) and (ny < 9 or leap[8])          # 1896 and 1904 are leap, 1900 is not
        got = t.rec.cols.reshape(ny, 12)
        for y in range(ny):
            assert got[y].tolist() == ((12 + np.arange(12)) if leap[y] else (12 * y + np.arange(12)) // ny).tolist()
            if not leap[y]:
                cols |= set(got[y].tolist())
        if ny == 13:
            assert set(got[~np.array(leap)].ravel().tolist()) == set(range(12))
        m = C.truth('tr', 'b', ny, True).rec.cols.reshape(ny, 12)
        assert all(m[y].tolist() == list(range(12 * leap[y], 12 * leap[y] + 12)) for y in range(ny))
    assert cols == set(range(12))


# ------------------------------------------------------------------------------------------- restatement = reference
def _against_reference(name, got, rec, ref, exact):
    """Classes and the sign of an exact zero; numbers equal where no transcendental decides them (``exact``); within two ulp
    of scale elsewhere (numpy's functions may differ in the last bit between CPUs)."""
    assert P.classes_equal(got, ref), name + ': classes differ'
    assert P.same(got[exact], ref[exact]), name + ': values differ where no transcendental is taken'
    fin = np.isfinite(ref)
    e = P.errors(got, ref.astype(P.LD), np.asarray(rec.scale, dtype=np.float64), ref)
    assert float(e[fin].max()) <= 2 * ULP, '{}: {:.3e} x scale off the reference'.format(name, float(e.max()))


@pytest.mark.parametrize('which', ['a', 'b'])
def test_restatement_is_the_reference_hargreaves(golden, which):
    g = golden('pet_edges')
    cs = C.cases('hg', which)
    rows = slice(None) if which == 'a' else C.GOLDEN_B_LATS
    got, rec = P.hargreaves(cs.temp[rows], cs.dtr[rows], cs.lat[rows], cs.dec, cs.dr, cs.nd)
    _against_reference('hargreaves ' + which, got, rec, g['hg_' + which], got == 0)


@pytest.mark.parametrize('which', ['a', 'b'])
def test_restatement_is_the_reference_hs(golden, which):
    g = golden('pet_edges')
    cs = C.cases('hs', which)
    rows = slice(None) if which == 'a' else C.GOLDEN_B_LATS
    got, rec = P.hs(cs.tas[rows], cs.tmax[rows], cs.tmin[rows], cs.lat[rows], cs.nd)
    ref = g['hs_' + which]
    _against_reference('hs ' + which, got, rec, ref, got == 0)
    cold = rec.branch == P.HS_COLD
    assert cold.any() and P.same_bits(ref[cold], np.zeros(int(cold.sum()))) and P.same_bits(got[cold], ref[cold])
    if which == 'b':                                        # tests/test_gpu_pet_ext.py keeps its own restatement: it is this one
        import test_gpu_pet_ext
        assert P.same_bits(test_gpu_pet_ext.hs_np(cs.tas, cs.tmax, cs.tmin, cs.lat, 1899, 1900),
                           P.hs(cs.tas, cs.tmax, cs.tmin, cs.lat, cs.nd)[0])


@pytest.mark.parametrize('which', ['a', 'b'])
def test_restatement_is_the_reference_daylight(golden, which):
    g = golden('pet_edges')
    lat = C.cases('dl', which).lat[slice(None) if which == 'a' else C.GOLDEN_B_LATS]
    ref = g['dl_' + which]
    for leap in (False, True):
        got, rec = P.daylight(lat, leap, order='numpy')
        r = ref[:, 12:] if leap else ref[:, :12]
        days = np.array(P.LEAP_MONTHDAYS if leap else P.MONTHDAYS)
        _against_reference('daylight ' + which, got, rec, r, (rec.lo + rec.hi == days))
        assert set(np.unique(got[(rec.lo == days) | (rec.hi == days)]).tolist()) == {0.0, 24.0}


def test_restatement_is_the_reference_thornthwaite(golden):
    g = golden('pet_edges')
    a = C.cases('tr', 'a')
    for y in C.YEARS_A:
        got, rec = P.thornthwaite(a.tas, a.lat, y, y, order='numpy')
        _against_reference('thornthwaite {}'.format(y), got, rec, g['tr_a_{}'.format(y)], got == 0)
    for ny in C.NYEARS_B:
        b = C.cases('tr', 'b', ny)
        got, rec = P.thornthwaite(b.tas[C.GOLDEN_B_CELLS], b.lat[C.GOLDEN_B_CELLS], C.Y0_B, C.Y0_B + ny - 1, order='numpy')
        _against_reference('thornthwaite B {}'.format(ny), got, rec, g['tr_b_{}'.format(ny)], got == 0)
        import test_gpu_pet_ext
        assert P.same_bits(test_gpu_pet_ext.trn_np(b.tas, b.lat, C.Y0_B, C.Y0_B + ny - 1),
                           P.thornthwaite(b.tas, b.lat, C.Y0_B, C.Y0_B + ny - 1, order='numpy')[0])


# ------------------------------------------------------------------------------------------- the conditions of the bar
@pytest.mark.parametrize('stage,which', SETS)
def test_no_case_left_out_and_branches_agree(stage, which):
    for key in C.runs(stage, which):
        t = C.truth(stage, which, *key)
        assert not t.left_out.any(), 'left out: ' + str(np.argwhere(t.left_out)[:5])
        for h, name in zip(t.hosts, P.hooks(C.STAGE[stage])):
            assert np.array_equal(h[1].branch, t.rec.branch), 'float64 ({}) and long double take different branches'.format(name)
    # the smallest gap that is not an exact tie is the 1e-6 margin, or what the grid happens to hold
    t = C.truth(stage, which, *C.runs(stage, which)[0])
    gap = np.asarray(t.rec.gap, dtype=np.float64)
    print('{} {}: smallest gap {:.3e}'.format(stage, which, gap[gap > 0].min()))
    assert gap[gap > 0].min() > 1e-8


@pytest.mark.parametrize('stage,which', SETS)
def test_bar(stage, which):
    """E_host: the worst |float64 restatement - long-double truth| / scale, the plain restatement and every one-ulp nudge."""
    e = C.e_host(stage, which)
    print('{} {}: E_host = {:.3e} = {:.1f} ulp of scale; bar {:.3e}'.format(stage, which, e, e / ULP, C.bar(stage, which)))
    assert 2.0 ** -54 < e <= GWAM_WORST
    for key in C.runs(stage, which):
        t = C.truth(stage, which, *key)
        for h in t.hosts:
            assert P.classes_equal(h[0], t.host)
            assert C.worst(h[0], t) <= e


def test_a_wrong_constant_is_far_above_the_bar():
    """17.8 -> 17.8 (1 + 1e-9) moves PET by 1e-9 x 17.8 / (t + 17.8): thousands of bars."""
    for stage, cs_t in (('hg', 'temp'), ('hs', 'tas')):
        t = C.truth(stage, 'b')
        ok = np.isfinite(t.host) & (t.host > 0)
        shift = np.abs(t.host[ok]) * 1e-9 * 17.8 / np.abs(getattr(t.cs, cs_t)[ok] + 17.8)
        assert np.median(shift / np.asarray(t.scale, dtype=np.float64)[ok]) > 1e3 * C.bar(stage, 'b')


# ------------------------------------------------------------------------------------------- why bits are not asserted
def test_summation_orders_differ_in_bits_yet_both_are_right():
    """The device adds a year's twelve pow() and a month's days one after the other, np.add.reduceat with eight accumulators:
    the results differ in the last bits of many rows, and both are as close to the truth as float64 gets."""
    t = C.truth('dl', 'b')
    seq, npy = t.host, t.run(np.float64, None, 'numpy')[0]
    differ = (seq != npy) & np.isfinite(seq)
    print('daylight: {} of {} table entries differ between the orders'.format(int(differ.sum()), differ.size))
    assert differ.mean() > 0.1
    assert C.worst(npy, t) <= C.e_host('dl', 'b') and C.worst(seq, t) <= C.e_host('dl', 'b')
    for monthly in (False, True):
        t = C.truth('tr', 'b', 13, monthly)
        seq, (npy, rec) = t.host, t.run(np.float64, None, 'numpy')
        I_seq = t.hosts[0][1].I
        print('thornthwaite: I differs in {} of {} years, PET in {} of {} months'.format(
            int((I_seq != rec.I).sum()), I_seq.size, int((seq != npy).sum()), seq.size))
        assert (I_seq != rec.I).mean() > 0.2 and (seq != npy).mean() > 0.2
        assert C.worst(npy, t) <= C.e_host('tr', 'b') and C.worst(seq, t) <= C.e_host('tr', 'b')
