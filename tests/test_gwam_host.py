"""CPU tests of the GWAM test apparatus itself (tests/gwam_np.py, tests/gwam_cases.py): that the case sets reach every
decision and every row shift, that the numpy restatement is the reference's runoffgen, that no case sits where GWAM is
discontinuous, and what error a correct float64 GWAM has against the long-double truth -- the bar tests/test_gpu_gwam.py
holds the device kernel to.  No GPU, no reference tree: the reference's outputs come from tests/golden/gwam_edges.npz.
"""
import numpy as np
import pytest

import gwam_cases as C
import gwam_np as G
from gwam_np import A_TMP3, FULL, LAKE, NANB, NOSOIL, PART, S_LE0, S_SM, T5_GE1, T5_LE01

# Every decision combination of the partial branch that inputs can be built to reach.  tmp5 >= 1 and tmp5 <= 0.1 exclude each
# other; Sm <= tmp8 and Sav <= 0 exclude each other (Sm > 0).  Of the 18 that leaves, four cannot be built:
#   tmp5 >= 1 (1 <= x <= 1.5) with Sav <= 0, AET = tmp7:  tmp8 = ch g(x) + P - PET > ch + P - PET > 0 as g(x) >= 1 there
#   tmp5 >= 1 with Sav <= 0, AET = tmp3:                  tmp8 = ch (g(x) - 1) >= 0, zero at x = 1 alone, where rounding decides
#   tmp5 >= 1 with Sm <= tmp8, AET = tmp3:                tmp8 = ch (g(x) - 1) <= 0.23 ch < Sm for x <= 1.5
#   0.1 < tmp5 < 1 ... none;  tmp5 <= 0.1 with Sav <= 0, AET = tmp7 needs x < 0.0607 (from above 2.4385, g > 1) -- same code
# with g(x) = (1 - exp(-x)) / (1 - exp(-1)).  tmp5 <= 0.1 with AET = tmp3 and 0 < tmp8 < Sm needs 2.4385 < x with
# x (g(x) - 1) < 1, which no x satisfies: set A reaches it through P = -inf (tmp8 = NaN compares false both ways).
PART_CODES_A = [
    PART, PART | T5_GE1, PART | T5_LE01,
    PART | A_TMP3, PART | T5_GE1 | A_TMP3, PART | T5_LE01 | A_TMP3,
    PART | S_SM, PART | T5_GE1 | S_SM, PART | T5_LE01 | S_SM,
    PART | A_TMP3 | S_SM, PART | T5_LE01 | A_TMP3 | S_SM,
    PART | S_LE0, PART | T5_LE01 | S_LE0,
    PART | A_TMP3 | S_LE0, PART | T5_LE01 | A_TMP3 | S_LE0,
]
# Set B's initial storage is Sm x {0, 0.05, 0.5, 1, 1.3, 2.6} and Sav <= Sm afterwards, so x never lies in (1.5, 2.4385):
# 0.1 < tmp5 < 1 with AET = tmp3 and tmp8 > 0 (x > 1 there) is out of its reach, and it has no infinite forcing.
PART_CODES_B = [c for c in PART_CODES_A if c not in (PART | A_TMP3, PART | A_TMP3 | S_SM, PART | T5_LE01 | A_TMP3)]
KINDS = [NOSOIL, LAKE, NANB, FULL]


def _missing(want, codes):
    have = set(np.unique(codes).tolist())
    return [G.describe(c) for c in want if c not in have]


def test_long_double_is_extended():
    assert np.finfo(G.LD).nmant >= 63


def test_branch_coverage_a():
    t = C.truth_a()
    assert not _missing(KINDS + PART_CODES_A, t.rec.code)
    # the grid alone (without the hand-written rows) reaches every partial combination that finite inputs reach
    grid = t.cs.label == 'grid'
    assert not _missing([c for c in PART_CODES_A if c != (PART | T5_LE01 | A_TMP3)], t.rec.code[grid])
    # storage above capacity: the clamp binds, tmp5 falls below 0.1 from above and below 0
    x = t.cs.ch[grid] / t.cs.sm[grid]
    part = (t.rec.code[grid] & G.KIND_MASK) == PART
    code = t.rec.code[grid]
    assert (part & (x > 1) & (x < 1.5) & (code & T5_GE1 != 0)).any()
    assert (part & (x > 2.4385) & (x < 2.5) & (code & T5_LE01 != 0)).any() and (part & (x > 2.5)).any()
    assert (part & (x > 1.5) & (x < 2.4385) & (code & (T5_GE1 | T5_LE01) == 0)).any()
    alt = C.truth_a(alt=True)
    assert not _missing([LAKE, NOSOIL, FULL, PART], alt.rec.code & G.KIND_MASK)
    # 999 is soil under the other code
    assert (alt.rec.code[alt.cs.sm == 999.0] & G.KIND_MASK != LAKE).all()


def test_branch_coverage_b():
    codes = []
    for monthly in (True, False):
        for spinup in (0, 12):
            r = C.truth_b(monthly, spinup).rec
            codes += [r.code.ravel(), r.spin_code.ravel()]
            assert not _missing(KINDS + PART_CODES_B, np.concatenate(codes[-2:])), (monthly, spinup)


def test_shift_coverage():
    want = set(range(0, 16, 2))
    # set B: every shift, every row over four tiles
    s = C.shifts(C.NC_B, C.NM_B)
    assert set(s.tolist()) == want and (C.tiles_spanned(s, C.NM_B) >= 3).all()
    # set C: every shift on rows over at least three tiles, for the shapes together and for the placed rows
    seen = set()
    for nm, nc in C.shapes_c():
        s = C.shifts(nc, nm)
        seen |= set(s[C.tiles_spanned(s, nm) >= 3].tolist())
    assert seen == want
    s = (np.array(C.ROWS_C) * C.NM_B) % C.TMS
    assert set(s.tolist()) == want
    # ... and the tail tile (the kernel's ntiles-th): reached at every shift by the long rows, and by some rows but not by
    # others at the lengths where a small shift ends a row one tile early
    for nm in C.NMONTHS_C:
        s = C.shifts(257, nm)
        ntiles = (nm + 14 + 15) // 16
        reach = C.tiles_spanned(s, nm) == ntiles
        assert (C.tiles_spanned(s, nm) <= ntiles).all()
        if nm in (34, 50):
            assert set(s[reach].tolist()) == want
        if nm in (14, 30):
            assert reach.any() and not reach.all()
        if nm == 16:                                        # every row unshifted: the tail tile holds no month at all
            assert not s.any() and not reach.any()
    # the shape list holds the shapes the launch can go wrong at: one cell, a last wave of one cell, 31 / 32 / 33
    assert {1, 31, 32, 33, 65, 257} <= set(C.NCELL_C) and {2, 14, 16, 18} <= set(C.NMONTHS_C)


def _against_reference(name, got, ref, code, scale):
    """Bits where no exp was evaluated; 2 x 2^-53 x scale elsewhere (numpy's exp may differ in the last bit between CPUs)."""
    noexp = (code & G.KIND_MASK) != PART
    sc = np.broadcast_to(scale[:, None] if ref.ndim == 2 else scale, ref.shape)
    assert G.same_bits(got[noexp], ref[noexp]), name + ': bits differ where no exp is taken'
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name + ': NaN masks differ'
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]) and np.array_equal(np.isinf(got), inf), name + ': infinities differ'
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin]) / sc[fin]
    assert err.max() <= 2 * 2.0 ** -53, '{}: {:.3e} x scale off the reference'.format(name, float(err.max()))


@pytest.mark.parametrize('tag', ['a', 'alt'])
def test_restatement_is_the_reference_one_month(golden, tag):
    g = golden('gwam_edges')
    t = C.truth_a(alt=tag == 'alt')
    cs = t.cs
    for k in ('ch', 'p', 'pet', 'sm'):                      # the fixture was made from these very inputs
        assert G.same_bits(getattr(cs, k), g[tag + '_' + k]), k
    got = G.month(cs.pet, cs.p, cs.sm, cs.ch, np.float64, None, cs.indexing)
    for i, k in enumerate(('aet', 'q', 'sav')):
        _against_reference(tag + ' ' + k, got[i], g[tag + '_' + k], got[3].code, t.scale)
    # tests/test_gpu_hgm.py keeps its own float64 restatement for its own bounds: it is this one, bit for bit
    if tag == 'a':
        import test_gpu_hgm
        for x, y in zip(test_gpu_hgm.gwam_month_np(cs.pet, cs.p, cs.sm, cs.ch), got[:3]):
            assert G.same_bits(x, y)


@pytest.mark.parametrize('mode', ['ref', 'mon'])
def test_restatement_is_the_reference_marched(golden, mode):
    g = golden('gwam_edges')
    b = C.set_b()
    idx = g['b_cells']
    assert np.array_equal(idx, C.GOLDEN_B_CELLS)
    pet, precip, sm, sm0 = g['b_pet'], g['b_precip'], g['b_sm'], g['b_sm0']
    for x, y in ((pet, b.pet[idx]), (precip, b.precip[idx]), (sm, b.sm[idx]), (sm0, b.sm0[idx])):
        assert G.same_bits(x, y)
    got = G.series(pet, precip, sm, sm0, int(g['b_spinup']), mode == 'mon')
    scale = C.scale_b(b)[idx]
    # a month is "without exp" for a cell only if no month before it, in either pass, took the partial branch
    part = (got[3].code & G.KIND_MASK) == PART
    spun = ((got[3].spin_code & G.KIND_MASK) == PART).any(axis=1)
    tainted = (np.cumsum(part, axis=1) > 0) | spun[:, None]
    code = np.where(tainted, PART, got[3].code)
    for i, k in enumerate(('aet', 'q', 'sav')):
        ref = g['b_{}_{}'.format(mode, k)]
        _against_reference(mode + ' ' + k, got[i], ref, code, scale)
    import test_gpu_hgm
    for x, y in zip(test_gpu_hgm.gwam_series_np(pet, precip, sm, sm0, int(g['b_spinup']), mode == 'mon'), got[:3]):
        assert G.same_bits(x, y)


def test_no_case_on_a_discontinuity():
    a = C.truth_a()
    assert not a.left_out.any(), 'set A may leave out no cell: ' + str(np.nonzero(a.left_out)[0][:10])
    assert not C.truth_a(alt=True).left_out.any()
    # exact ties with B == Sm are the hand-written ones
    tie = a.rec.gap_b == 0
    assert tie.any() and set(a.cs.label[tie].tolist()) <= {'tie B == Sm', 'negative zero'}
    for monthly in (True, False):
        for spinup in C.SPINUPS_B:
            for constant in ((False, True) if monthly else (False,)):
                t = C.truth_b(monthly, spinup, constant)
                share = t.left_out.mean()
                print('set B monthly={} spinup={} constant={}: {} of {} cells left out'.format(
                    monthly, spinup, constant, int(t.left_out.sum()), t.left_out.size))
                assert share <= 0.02


def test_bar():
    """E_host: the worst |float64 restatement - long-double truth| / scale over numpy's exp and exp moved one ulp either way."""
    a = C.truth_a()
    print('set A: E_host = {:.3e} = {:.1f} ulp of scale; bar {:.3e}'.format(a.e_host, a.e_host / 2.0 ** -53, a.bar))
    # a correct float64 GWAM month is a handful of roundings: anything beyond 2^-49 would mean the restatement or the truth
    # is wrong, anything below 2^-54 that the two are the same arithmetic
    assert 2.0 ** -54 < a.e_host < 2.0 ** -49
    worst = 0.0
    for monthly in (True, False):
        for spinup in C.SPINUPS_B:
            t = C.truth_b(monthly, spinup)
            worst = max(worst, t.e_host)
            print('set B monthly={} spinup={}: E_host = {:.3e} = {:.1f} ulp of scale; bar {:.3e}'.format(
                monthly, spinup, t.e_host, t.e_host / 2.0 ** -53, t.bar))
            # up to 100 months marched: no more than a month's error per month
            assert 2.0 ** -54 < t.e_host < 100 * 2.0 ** -49
            # the three host runs differ from each other by rounding luck alone: each stays inside the bar of 4 x the worst
            for h in t.hosts:
                for x, y in zip(h, t.truth):
                    assert G.worst_error(x, y, t.scale, ~t.left_out) <= t.bar
    # a wrong constant is orders of magnitude above the bar: 0.1 -> 0.1 (1 + 1e-9) moves AET by 1e-10 x PET
    cs = a.cs
    floor = (a.rec.code & (T5_LE01 | A_TMP3 | S_LE0) == T5_LE01) & ((a.rec.code & G.KIND_MASK) == PART) & np.isfinite(cs.pet)
    assert floor.any() and (1e-10 * np.abs(cs.pet[floor]) / a.scale[floor]).max() > 1e3 * a.bar
