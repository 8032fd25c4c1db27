"""GPU tests of the GWAM kernels (csrc/xh_gwam.hip: gwam_month, k_gwam_spinup, k_gwam_tile) at every branch, tie and row
shift, against a long-double numpy truth (tests/gwam_np.py) on the case sets of tests/gwam_cases.py.

The bar is not a literal: tests/gwam_cases.py computes E_host, the worst |float64 restatement - long-double truth| / scale
of a correct float64 GWAM (numpy's exp, and exp moved one ulp either way), and the device is held to 4 x E_host, per set
and per run, against the long-double truth.  Bits are asserted only where the arithmetic has no exp in it.

Measured on an MI355X (worst over AET, Q, Sav and sm_end; printed by the tests).  No cell is left out of any run (the
condition is at most 2 % of set B and none of set A); no defect was found in the kernel or the wrapper.

    set, run                     E_host (x scale)   bar = 4 E_host   device error   error / bar
    A (2,850 + 62 + 10 rows)     3.95e-16  3.6 ulp  1.58e-15         3.95e-16       0.250
    B monthly,   spin-up 0       1.24e-15 11.2 ulp  4.98e-15         1.16e-15       0.233
    B monthly,   spin-up 12      5.93e-16  5.3 ulp  2.37e-15         5.35e-16       0.225
    B monthly,   spin-up 50      6.03e-16  5.4 ulp  2.41e-15         2.42e-16       0.100
    B reference, spin-up 0       3.64e-15 32.8 ulp  1.46e-14         6.93e-16       0.048
    B reference, spin-up 12      3.64e-15 32.8 ulp  1.46e-14         8.27e-16       0.057
    B reference, spin-up 50      1.77e-15 16.0 ulp  7.10e-15         3.39e-16       0.048

Mutation check (not committed; one comparison or constant of gwam_month changed at a time in a scratch build of the
library, this file run against each):

    0.1 -> 0.11 (the floor of tmp6)      test_set_a_within_bar, test_set_b_within_bar (all six runs)
    B >= sm -> B > sm                    test_set_a_within_bar, test_set_a_bits_where_no_exp, test_exact_values_at_clamps_and_ties
                                         (the three `tie B == Sm` rows fall into no branch and come out 0)
    else if (B < sm) -> else             the same three and test_set_b_within_bar: a NaN B marches through the partial branch
    s <= 0.0 -> s < 0.0                  none, and no input of these sets can: the two differ only at tmp8 == +-0 with
                                         AET = tmp7 < tmp3.  With ch = 0, tmp8 = P - AET is 0 only when AET = tmp3 = P, where
                                         both sides write AET = P + ch, Sav = +0, Q = 0 (rows `tie tmp8 == 0`, `tie ch = P = 0`);
                                         tmp8 = -0 needs ch = P = -0, which gives AET = tmp3 = -0 and tmp8 = +0 (rows
                                         `negative zero`).  With ch > 0 the sum ch (1 - exp(-x)) / k1 + (P - AET) would have to
                                         cancel to exactly 0 through the last bit of exp, which no portable input fixes.
    drop `|| tmp3 != tmp3`               none: dead code.  tmp3 = ch + P is NaN only when B = ch + P - PET is NaN, and a NaN B
                                         never reaches the partial branch (rows `ch NaN`, `P NaN soil`, `inf`)
    1.0 <= tmp5 -> 1.0 < tmp5            none: at the tie both sides return 1.0 (rows `tie tmp5 == 1`); the same holds for
                                         every other tie of a minimum or maximum of two equal numbers
"""
import itertools

import numpy as np
import pytest

import gwam_cases as C
import gwam_np as G

pytestmark = pytest.mark.gpu

GUARD = 16                                                 # doubles before and after every output allocation
SENTINEL = np.uint64(0x7ff8dead0000beef)                   # a NaN no arithmetic makes
OUTS = ('aet', 'q', 'sav')


class Result(dict):
    __getattr__ = dict.__getitem__


def run(pet, precip, sm, sm0, spinup, mode, indexing=999.0, outputs=OUTS, sm_end=True, guard=GUARD):
    """xh_gwam through the C ABI on host arrays.  Every output sits inside a larger allocation filled with a sentinel;
    nothing outside [0, ncell x nmonths) of it may be written.  Outputs not in ``outputs`` are passed as NULL."""
    from xanthos_amd import _hip
    from xanthos_amd.runoff import gwam
    ctx = _hip.get_context(0)
    pet = np.ascontiguousarray(pet, dtype=np.float64)
    ncell, nmonths = pet.shape
    cs, cm = gwam.precip_columns(mode, spinup, nmonths)
    ins = [ctx.upload(a) for a in (pet, np.ascontiguousarray(precip, dtype=np.float64), np.asarray(sm, dtype=np.float64),
                                   np.asarray(sm0, dtype=np.float64))]
    sizes = {k: ncell * nmonths for k in outputs}
    if sm_end:
        sizes['sm_end'] = ncell
    bufs = {k: ctx.upload(np.full(n + 2 * guard, SENTINEL, dtype=np.uint64).view(np.float64)) for k, n in sizes.items()}
    ptr = lambda k: bufs[k].ptr + 8 * guard if k in bufs else None          # noqa: E731
    try:
        ctx.gwam(ncell, nmonths, spinup, cs, cm, indexing, *ins, ptr('aet'), ptr('q'), ptr('sav'), ptr('sm_end'))
        ctx.sync()
        res = Result()
        for k, n in sizes.items():
            raw = bufs[k].download()
            edge = np.concatenate([raw[:guard], raw[guard + n:]]).view(np.uint64)
            assert (edge == SENTINEL).all(), k + ': written outside the array'
            body = raw[guard:guard + n]
            assert not (body.view(np.uint64) == SENTINEL).any(), k + ': elements left unwritten'
            res[k] = body.copy() if k == 'sm_end' else body.reshape(ncell, nmonths).copy()
    finally:
        for b in ins + list(bufs.values()):
            b.free()
    return res


def run_cs(cs, spinup, mode, **kw):
    return run(cs.pet, cs.precip, cs.sm, cs.sm0, spinup, mode, cs.indexing, **kw)


def two(a):
    return np.repeat(np.asarray(a, dtype=np.float64).reshape(-1, 1), 2, axis=1)


_runs = {}


def run_a(alt=False):
    """Set A as a two-month `monthly` call with the month duplicated (the kernel marches pairs of months)."""
    if alt not in _runs:
        cs = C.truth_a(alt).cs
        _runs[alt] = run(two(cs.pet), two(cs.p), cs.sm, cs.ch, 0, 'monthly', cs.indexing)
    return _runs[alt]


def run_b(monthly, spinup, constant=False):
    key = (monthly, spinup, constant)
    if key not in _runs:
        _runs[key] = run_cs(C.truth_b(monthly, spinup, constant).cs, spinup, 'monthly' if monthly or constant else 'reference')
    return _runs[key]


def assert_same(a, b, what=''):
    for k in a:
        assert G.same_bits(a[k], b[k]), '{} {}: bits differ'.format(what, k)


# ------------------------------------------------------------------------------------------- 1. within the bar of the truth
@pytest.mark.parametrize('alt', [False, True])
def test_set_a_within_bar(alt):
    t, r = C.truth_a(alt), run_a(alt)
    assert not t.left_out.any()
    worst = max(G.worst_error(r[k][:, 0], t.truth[i], t.scale) for i, k in enumerate(OUTS))
    print('set A{}: worst error {:.3e} x scale, bar {:.3e}, ratio {:.3f}'.format(' (alt)' if alt else '', worst, t.bar,
                                                                               worst / t.bar))
    assert worst <= t.bar
    # the second month starts from the first month's Sav, and sm_end is its Sav
    cs = t.cs
    again = G.month(cs.pet, cs.p, cs.sm, r.sav[:, 0], G.LD, None, cs.indexing)
    near = C.near_discontinuity(again[3].gap_b, t.scale) | C.near_discontinuity(again[3].gap_8, t.scale)
    for i, k in enumerate(OUTS):
        assert G.worst_error(r[k][:, 1], again[i], t.scale, ~near) <= t.bar
    assert G.same_bits(r.sm_end, r.sav[:, 1])


@pytest.mark.parametrize('spinup', C.SPINUPS_B)
@pytest.mark.parametrize('mode', ['monthly', 'reference'])
def test_set_b_within_bar(mode, spinup):
    t, r = C.truth_b(mode == 'monthly', spinup), run_b(mode == 'monthly', spinup)
    assert t.left_out.mean() <= 0.02
    keep = ~t.left_out
    worst = max(G.worst_error(r[k], t.truth[i], t.scale, keep) for i, k in enumerate(OUTS + ('sm_end',)))
    print('set B {} spinup {}: worst error {:.3e} x scale, bar {:.3e}, ratio {:.3f}, {} cells left out'.format(
        mode, spinup, worst, t.bar, worst / t.bar, int(t.left_out.sum())))
    assert worst <= t.bar


# ------------------------------------------------------------------------------------------- 2. bits without a transcendental
@pytest.mark.parametrize('alt', [False, True])
def test_set_a_bits_where_no_exp(alt):
    t, r = C.truth_a(alt), run_a(alt)
    host = t.hosts[0]
    noexp = (host[3].code & G.KIND_MASK) != G.PART
    assert noexp.sum() > (4 if alt else 1400)
    for kind in (G.NOSOIL, G.LAKE, G.NANB, G.FULL):
        m = (host[3].code & G.KIND_MASK) == kind
        assert m.any() or alt
        for i, k in enumerate(OUTS):
            assert G.same_bits(r[k][m, 0], host[i][m]), '{} on {} cells'.format(k, G.KIND_NAMES[kind])
    # which NaN inputs give 0 and which give NaN, spelled out
    if not alt:
        lab = t.cs.label
        for name in ('Sm NaN', 'ch NaN', 'PET NaN soil', 'P NaN soil', 'no soil'):
            for k in OUTS:
                assert G.same_bits(r[k][lab == name, 0], np.zeros(int((lab == name).sum()))), (name, k)
        lake = np.nonzero(lab == 'lake NaN')[0]
        assert r.aet[lake[0], 0] == 5.0 and np.isnan(r.aet[lake[1:3], 0]).all() and r.aet[lake[3], 0] == 5.0
        assert G.same_bits(r.q[lake, 0], [0.0, 0.0, 0.0, 4.0]) and G.same_bits(r.sav[lake, 0], np.zeros(4))


# ------------------------------------------------------------------------------------------- 3. exact values at clamps and ties
def test_exact_values_at_clamps_and_ties():
    t, r = C.truth_a(), run_a()
    cs = t.cs
    runs = [t.truth] + [h[:3] for h in t.hosts]
    # a clamp that the long-double truth and the float64 restatement under all three exps agree on is not a matter of
    # rounding: the kernel has it exactly
    for k, i in (('q', 1), ('sav', 2)):
        zero = np.all([x[i] == 0 for x in runs], axis=0)
        assert zero.sum() > 300 and (r[k][zero, 0] == 0).all(), k + ' == 0'
    full = np.all([x[2] == cs.sm for x in runs], axis=0) & (cs.sm != 0)
    assert full.sum() > 1400 and G.same_bits(r.sav[full, 0], cs.sm[full]), 'Sav == Sm'
    sat = full & ((t.rec.code & G.KIND_MASK) == G.PART)                     # saturated through min(Sm, tmp8)
    assert sat.sum() > 50
    # the hand-written ties: AET and Q take no rounding of exp on any of them, Sav only where it is neither 0 nor Sm
    host = t.hosts[0]
    tie = np.char.startswith(cs.label, 'tie')
    assert tie.sum() == 13
    assert G.same_bits(r.aet[tie, 0], host[0][tie]) and G.same_bits(r.q[tie, 0], host[1][tie])
    clamp = tie & ((host[2] == 0) | (host[2] == cs.sm))
    assert G.same_bits(r.sav[clamp, 0], host[2][clamp])
    by = lambda name: np.nonzero(cs.label == name)[0]                      # noqa: E731
    # B == Sm is the full branch (>=): AET = PET, Q = +0, Sav = Sm
    for j in by('tie B == Sm'):
        assert (r.aet[j, 0], r.sav[j, 0]) == (cs.pet[j], cs.sm[j]) and G.same_bits(r.q[j, 0], 0.0)
    # tmp3 == tmp7: either side is the same number; Q = 0 because AET = ch + P
    for j in by('tie tmp3 == tmp7'):
        assert r.aet[j, 0] == cs.ch[j] + cs.p[j] == cs.pet[j] and r.q[j, 0] == 0 and 0 < r.sav[j, 0] < cs.sm[j]
    # tmp5 == 1: min(1, tmp5) = 1 from either side, AET = PET exactly
    for j in by('tie tmp5 == 1'):
        assert r.aet[j, 0] == cs.pet[j]
    # P == PET on a lake: AET = P, Q = +0
    for j in by('tie P == PET lake'):
        assert G.same_bits(r.aet[j, 0], cs.p[j]) and G.same_bits(r.q[j, 0], 0.0) and G.same_bits(r.sav[j, 0], 0.0)
    # ch = P = 0 and tmp8 == 0: Sav <= 0 includes 0 -- Sav = +0, AET = P + ch, Q = 0
    for j in list(by('tie ch = P = 0')) + list(by('tie tmp8 == 0')):
        assert G.same_bits(r.sav[j, 0], 0.0) and G.same_bits(r.aet[j, 0], cs.p[j] + cs.ch[j]) and G.same_bits(r.q[j, 0], 0.0)


# ------------------------------------------------------------------------------------------- 4. state
@pytest.mark.parametrize('mode', ['monthly', 'reference'])
def test_state(mode):
    monthly = mode == 'monthly'
    cs = C.set_b()
    for spinup in C.SPINUPS_B:
        r = run_b(monthly, spinup)
        assert G.same_bits(r.sm_end, r.sav[:, -1]), 'sm_end is the last Sav column'
    # spin-up k = a k-month run with the spin-up pass's precipitation, then a run without spin-up from its end state
    for k in (12, 50):
        head = run(cs.pet[:, :k], cs.precip[:, :k], cs.sm, cs.sm0, 0, mode, outputs=())
        tail = run(cs.pet, cs.precip, cs.sm, head.sm_end, 0, mode)
        assert_same(tail, run_b(monthly, k), 'spin-up {}'.format(k))
    # and spin-up = nmonths is not spin-up = 0
    assert not G.same_bits(run_b(monthly, 50).sav, run_b(monthly, 0).sav)


# ------------------------------------------------------------------------------------------- 5. invariance in bits
def test_constant_columns_monthly_is_reference():
    """With every precipitation column equal, month m's column is the one column `reference` reads in either pass."""
    cs = C.constant_precip(C.set_b())
    for spinup in C.SPINUPS_B:
        assert_same(run_b(True, spinup, constant=True), run_cs(cs, spinup, 'reference'), 'spin-up {}'.format(spinup))
    # without spin-up, `reference` on set B itself reads the last column only: the same march again
    assert_same(run_b(True, 0, constant=True), run_b(False, 0))


@pytest.mark.parametrize('base', [7, 13, 58, 466])
def test_same_row_at_every_cell_index(base):
    """One row of B at twelve cell indices of a 257-cell problem: eight shifts, first and last lanes, three waves."""
    b = C.set_b()
    cs = C.rows_for(b, 257, C.NM_B, first=600)
    for c in C.ROWS_C:
        cs.pet[c], cs.precip[c], cs.sm[c], cs.sm0[c] = b.pet[base], b.precip[base], b.sm[base], b.sm0[base]
    big = run_b(True, 0)
    for mode, spinup in (('monthly', 0), ('monthly', 12), ('reference', 12)):
        r = run_cs(cs, spinup, mode)
        for k in OUTS:
            for c in C.ROWS_C:
                assert G.same_bits(r[k][c], r[k][0]), '{} row at cell {} ({} spin-up {})'.format(k, c, mode, spinup)
        assert G.same_bits(r.sm_end[list(C.ROWS_C)], np.full(len(C.ROWS_C), r.sm_end[0]))
        if (mode, spinup) == ('monthly', 0):                # ... and what it gave at its own place in set B
            for k in OUTS:
                assert G.same_bits(r[k][0], big[k][base])


@pytest.mark.parametrize('nmonths', C.NMONTHS_C)
def test_every_shape_is_a_prefix_of_the_march(nmonths):
    """[ncell, nmonths] problems cut from B equal, in bits, the same rows and months of the 1,200 x 50 march: at every
    ncell, at every prefix length, and with the rows at other cell indices (hence other shifts) than in the march."""
    b = C.set_b()
    big = run_b(True, 0)
    for ncell in C.NCELL_C:
        first = (37 * ncell + nmonths) % 1000
        r = run_cs(C.rows_for(b, ncell, nmonths, first), 0, 'monthly')
        idx = (first + np.arange(ncell)) % b.ncell
        for k in OUTS:
            assert G.same_bits(r[k], big[k][idx, :nmonths]), '{} at {} cells x {} months'.format(k, ncell, nmonths)
        assert G.same_bits(r.sm_end, big.sav[idx, nmonths - 1])


@pytest.mark.parametrize('mode,spinup', [('monthly', 0), ('reference', 12)])
def test_null_outputs(mode, spinup):
    """Every subset of the three outputs NULL, sm_end given or not: what is given has the bits of the full run, and
    nothing is written outside it (``run`` checks the guard elements of every allocation)."""
    cs = C.rows_for(C.set_b(), 65, 34, first=100)
    want = run_cs(cs, spinup, mode)
    for n in range(4):
        for outs in itertools.combinations(OUTS, n):
            for end in (True, False):
                r = run_cs(cs, spinup, mode, outputs=outs, sm_end=end)
                assert set(r) == set(outs) | ({'sm_end'} if end else set())
                assert_same(r, want, 'outputs {} sm_end {}'.format(outs, end))


def test_outputs_only_16_byte_aligned():
    """The ABI asks for 16-byte alignment, not for whole lines: outputs 16 bytes off a line give the same bits."""
    cs = C.rows_for(C.set_b(), 33, 18, first=200)
    assert_same(run_cs(cs, 0, 'monthly', guard=2), run_cs(cs, 0, 'monthly'))
    assert_same(run_cs(cs, 12, 'reference', guard=18), run_cs(cs, 12, 'reference'))


# ------------------------------------------------------------------------------------------- 6. the Python entry points
def test_runoffgen_and_execute_give_the_abi_path():
    from xanthos_amd.runoff import gwam
    for alt in (False, True):
        cs, r = C.truth_a(alt).cs, run_a(alt)
        pet, aet, q, sav = gwam.runoffgen(cs.pet, cs.p, None, cs.sm, cs.ch, indexing=cs.indexing)
        assert G.same_bits(pet, cs.pet)
        for x, k in ((aet, 'aet'), (q, 'q'), (sav, 'sav')):
            assert G.same_bits(x, r[k][:, 0]), 'runoffgen ' + k
        pet, aet, q, sav = gwam.gwam_execute(two(cs.pet), two(cs.p), cs.sm, cs.ch, 0, precipitation='monthly',
                                             indexing=cs.indexing)
        for x, k in ((aet, 'aet'), (q, 'q'), (sav, 'sav')):
            assert G.same_bits(x, r[k]), 'gwam_execute ' + k
    b = C.set_b()
    for mode, spinup in (('reference', 12), ('monthly', 50)):
        _, aet, q, sav = gwam.gwam_execute(b.pet, b.precip, b.sm, b.sm0, spinup, precipitation=mode)
        want = run_b(mode == 'monthly', spinup)
        for x, k in ((aet, 'aet'), (q, 'q'), (sav, 'sav')):
            assert G.same_bits(x, want[k]), 'gwam_execute {} {}'.format(mode, k)
