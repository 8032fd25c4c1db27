"""The device math primitives bit for bit, and ABCD over the whole calibration box (-m gpu).

Part 1 runs every hand-written primitive of csrc/xh_math.h and csrc/xh_abcd_dev.h through the test-only probe library
(tests/math_probe: one element-wise kernel per call) and holds it to the claim written next to it: xh_exp equal in bits to
the device library's exp, xh_sqrt to IEEE sqrt, quot() to the IEEE quotient, abcd_split to the oracle's split, and the two
approximate ones (xh_exp_nonpos, frcp / fdiv) to their stated error against the true value.

Part 2 compares the ABCD month update in bits.  Every operation of it except exp is an IEEE operation in the reference's
order, so with the device's own exp values handed to the oracle (oracle.abcd._march(decay=...)) the device march must equal
it bit for bit at ANY parameters -- the corners of the box calibration searches included, where the stage bar
(1e-9 |ref| + 1e-9) is at once too loose to see a wrong rounding and too tight for a correct kernel
(test_math_host.py::test_why_the_march_is_compared_in_bits).  First the shared month update through the probe, then the
runoff kernels through the C-ABI at every launch shape, then the calibration objective.

"Equal in bits" is math_np.same_bits: identical NaN masks, identical bit patterns elsewhere (the sign of zero counts).

Measured on MI355X (gfx950, 256 CUs); the asserts hold the claims, these are the observed figures:
  xh_exp == exp() in bits ............ all 4,194,304 + 226,293 + 1,048,576 arguments; host build of the same source: same bits
  xh_exp / exp() against the true value  worst 0.8738 ulp (dense), 0.8633 (structured), 0.8286 (ABCD's arguments)
  xh_exp_nonpos ...................... worst 0.9463 of 1e-11 true + 2^-1074
  xh_sqrt == IEEE sqrt in bits ........ all 5.9 M arguments, 148,951 next to a rounding boundary among them
  quot == x / d in bits .............. every family; |x| < 2^-1000: 46,983 of 262,144 one step off, none more
  frcp / fdiv ........................ worst 11.11 / 18.31 ulp against the exact quotient
  bit comparisons of the march ....... all held: probe march (exact and FASTQ form, snow on / off), xh_abcd whole call at
                                       1 - 65 cells and over the box, the 32- / 40- / 48-cell waves, blocked = whole series,
                                       calibration series of a one-cell basin on both kernels
  infinite precipitation ............. NaN masks of device and oracle identical (the snowpack differs, NaN against inf, but
                                       rain = inf - inf is NaN on both sides in the same month)
  calibration objective at the corners  series 1.3e-2 of its 1e-9 bar at the worst, ED 8.9e-4 of it

Mutation check (done once on scratch copies, nothing of it kept): quot() as the bare product x * inv_d fails 40 of the 53
tests here (the quot, split, march, xh_abcd and calibration-series tests) while the 13 older ABCD and calibration-objective
tests of test_gpu_parity.py pass with the same mutated library; xh_sqrt without its last correction fails
test_xh_sqrt_is_ieee at 605 of the constructed arguments and nothing else -- no argument the march forms comes within
2^-43 of a step of a rounding boundary, so the march tests cannot see it, and before the constructed arguments were added
no test here could; the first coefficient of xh_exp changed in its last bit fails the three exp equalities.
"""
import numpy as np
import pytest

import math_np as M
from oracle import abcd as o_abcd

pytestmark = pytest.mark.gpu

# Worst error of frcp / fdiv against the exact quotient, measured on MI355X and rounded up to the next whole ulp: this is
# the figure written next to them in csrc/xh_math.h.  v_rcp_f64's accuracy is not specified to the last bit, so the bound
# comes from measurement; the structure behind it is in the test's docstring.
FRCP_BOUND_ULP = 12
FDIV_BOUND_ULP = 19


@pytest.fixture(scope='module')
def hip():
    from xanthos_amd import _hip
    assert _hip.device_count() > 0, 'no GPU visible'
    return _hip


@pytest.fixture(scope='module')
def probe():
    return M.probe()


def assert_bits(got, want, what, inputs=None):
    assert M.same_bits(got, want), '{}: {}'.format(what, M.describe_mismatch(got, want, inputs))


# =============================================================================================== part 1: primitives
@pytest.mark.parametrize('name', ['dense', 'structured', 'abcd'])
def test_xh_exp_is_the_library_exp(probe, name):
    """xh_exp == the device library's exp, in bits, over [-1080, 1030], every result class (+-0, +-inf, NaN, |x| < 2^-54,
    the selects at 1024 and -1075, subnormal results, arguments next to (n + 1/2) ln 2) and ABCD's own arguments
    -pet / b; the host compilation of the same source gives the same bits; and both are within 1 ulp of the true value.
    Measured: worst 0.874 ulp (dense), 0.863 (structured), 0.829 (ABCD's arguments)."""
    x = M.exp_inputs()[name]
    mine, lib = probe.unary(M.OP_XH_EXP, x), probe.unary(M.OP_LIB_EXP, x)
    assert_bits(mine, lib, 'xh_exp vs exp() on ' + name, (x,))
    assert_bits(probe.unary(M.OP_XH_EXP, x, host=True), mine, 'xh_exp on the host vs on the device', (x,))
    true = M.exp_true(x)
    over = true > np.finfo(np.float64).max
    ok = ~np.isnan(x) & ~over
    assert np.array_equal(np.isnan(mine), np.isnan(x)) and np.all(mine[over & ~np.isnan(x)] == np.inf)
    for tag, e in (('xh_exp', mine), ('exp', lib)):
        err = M.ulp_error(e[ok], true[ok])
        print('{} {}: worst {:.4f} ulp against the true value'.format(tag, name, float(err.max())))
        assert err.max() <= 1.0
    assert np.all(mine[x == 0.0] == 1.0) and np.all(mine[x > 1024.0] == np.inf) and np.all(mine[x < -1075.0] == 0.0)


def test_xh_exp_nonpos_claim(probe):
    """|e - true| <= 1e-11 true + 2^-1074 on [-1080, 0] and at -inf (the header's claim).  Measured worst ratio: 0.946."""
    x = M.exp_nonpos_inputs()
    e = probe.unary(M.OP_XH_EXP_NONPOS, x)
    true = M.exp_true(x)
    ratio = np.abs(e.astype(np.longdouble) - true) / (np.longdouble(1e-11) * true + np.longdouble(M.TINY))
    print('xh_exp_nonpos: worst ratio {:.4f}'.format(float(ratio.max())))
    assert not np.isnan(e).any() and ratio.max() <= 1.0
    assert np.all(e[x == -np.inf] == 0.0) and np.all(e[x == 0.0] == 1.0)
    assert_bits(probe.unary(M.OP_XH_EXP_NONPOS, x, host=True), e, 'xh_exp_nonpos on the host vs on the device', (x,))


def test_xh_sqrt_is_ieee(probe):
    """xh_sqrt == numpy.sqrt (IEEE, correctly rounded) in bits for +-0, +inf, NaN, negative arguments, log-uniform
    x in [2^-700, 2^1023], perfect squares and their neighbours; and so is the device library's sqrt."""
    x = M.sqrt_inputs()
    with np.errstate(invalid='ignore'):
        want = np.sqrt(x)
    assert_bits(probe.unary(M.OP_XH_SQRT, x), want, 'xh_sqrt vs numpy.sqrt', (x,))
    assert_bits(probe.unary(M.OP_LIB_SQRT, x), want, 'device sqrt vs numpy.sqrt', (x,))


def test_quot_is_the_ieee_quotient(probe):
    """quot(x, d, 1 / d) == numpy's x / d in bits for the three divisor families of the month update (1.9; 2a, 1000 b and
    d + 1 over the box) with numerators the march can form, divisors with all-ones / all-zeros mantissas, x = +0, and
    2^-960 <= |x| <= 2^1000; at most one step apart below 2^-1000; quot(-0.0, d) = +0.0 and quot(+-inf, d) = NaN as the
    header says.  The device's own IEEE division equals numpy's on the same inputs."""
    M.check_quot(lambda x, d: probe.binary(M.OP_QUOT, x, d))
    for name, (x, d) in M.quot_inputs().items():
        assert_bits(probe.binary(M.OP_IEEE_DIV, x, d), x / d, 'device x / d on ' + name, (x, d))


def test_frcp_fdiv_error(probe):
    """frcp(b) and fdiv(a, b) = a * frcp(b) against the EXACT quotient (extended precision on the sweep, fractions on a
    sample), for Penman-Monteith's magnitudes: |a|, |b| in [1e-6, 1e12], both signs.

    v_rcp_f64's accuracy is not specified to the bit, so no bound can be derived: the bounds are the worst cases measured
    on MI355X, rounded up to the next whole ulp -- frcp 11.11 -> 12 ulp, fdiv 18.31 -> 19 ulp (the product's ulp can be half
    the reciprocal's, so the same relative error counts double) -- and the same figures stand in csrc/xh_math.h.  Both
    are above the "few ulp" its comment used to promise (4 at the most): the comment was wrong and has been corrected."""
    from fractions import Fraction
    num, den = M.fdiv_inputs()
    r, qv = probe.unary(M.OP_FRCP, den), probe.binary(M.OP_FDIV, num, den)
    ld = np.longdouble
    e_r = M.ulp_error(r, ld(1.0) / den.astype(ld))
    e_q = M.ulp_error(qv, num.astype(ld) / den.astype(ld))
    print('frcp: worst {:.4f} ulp; fdiv: worst {:.4f} ulp (extended-precision reference, {} cases)'.format(
        float(e_r.max()), float(e_q.max()), num.size))
    worst = np.concatenate([np.argsort(e_q)[-500:], np.arange(1500)])
    fr = 0.0
    for i in worst:
        exact = Fraction(float(num[i])) / Fraction(float(den[i]))
        ulp = Fraction(float(np.spacing(abs(float(exact)))))
        fr = max(fr, float(abs(Fraction(float(qv[i])) - exact) / ulp))
    print('fdiv: worst {:.4f} ulp against the exact rational quotient on the sample'.format(fr))
    assert np.isfinite(r).all() and np.isfinite(qv).all()
    assert e_r.max() <= FRCP_BOUND_ULP
    assert e_q.max() <= FDIV_BOUND_ULP and fr <= FDIV_BOUND_ULP


@pytest.mark.parametrize('snow_on', [True, False])
def test_abcd_split_is_the_oracle_split(probe, snow_on):
    """abcd_split == oracle.abcd._split_rain_snow (rain, snow) and the melt fraction of _march's mixed class, in bits, with
    tmin on 0.6 and 2.5 and on both sides of each, NaN, +-inf, and precipitation 0, NaN and subnormal; without snow the
    rain is the precipitation and nothing melts."""
    precip, tmin = M.split_inputs()
    rain, snow, frac, kind = probe.split(snow_on, precip, tmin)
    if not snow_on:
        assert_bits(rain, precip, 'rain without snow')
        assert not snow.any() and not kind.any()
        return
    r_rain, r_snow, r_frac, r_kind, mixed = M.split_reference(precip, tmin)
    assert np.array_equal(kind, r_kind)
    assert mixed.sum() > 1 << 20 and (r_kind == 1).sum() > 1000 and (r_kind == 0).sum() > 1000
    assert_bits(rain, r_rain, 'rain', (precip, tmin))
    assert_bits(snow, r_snow, 'snow', (precip, tmin))
    assert_bits(frac[mixed], r_frac[mixed], 'melt fraction of the mixed class', (precip[mixed], tmin[mixed]))


# =============================================================================================== part 2: the month update
@pytest.fixture(scope='module')
def cases():
    return M.box_cases(nmonths=120)


def _init(n):
    return np.full(n, o_abcd.SM_INIT), np.full(n, o_abcd.GW_INIT)


@pytest.mark.parametrize('fastq', [False, True], ids=['exact', 'fastq'])
@pytest.mark.parametrize('snow_on', [True, False], ids=['snow', 'nosnow'])
def test_month_update_equals_oracle_in_bits(probe, cases, snow_on, fastq):
    """abcd_pre + abcd_step (the probe's march) against oracle.abcd._march with the probe's own decay injected: aet, q and
    sav equal in bits for the 32 corners of the calibration box, its 10 face centres, 2,000 random points of it and 500
    of today's range, under every forcing family of math_np.FORCINGS (all dry, 15 % and 30 % wet, pet = 0, pet = 1e4,
    NaN precipitation, NaN tmin, tmin on the thresholds, subnormal precipitation), 120 months.  The FASTQ form (the
    calibration marches) is held to the oracle with the groundwater line restated as (gw + c awet) * (1 / (d + 1))."""
    pars, pet, pr, tn, lab = cases
    tn = tn if snow_on else None
    sm0, gw0 = _init(len(pars))
    aet, q, sav, decay, _ = probe.march(pars, pet, pr, tn, sm0, gw0, fastq=fastq)
    # the decay itself: the device exp of the argument the form builds (checked so that a wrong argument cannot hide)
    b = pars[:, 1:2] * 1000
    arg = (-pet) * (1.0 / b) if fastq else probe.binary(M.OP_QUOT, -pet, np.broadcast_to(b, pet.shape)).reshape(pet.shape)
    assert_bits(decay, probe.unary(M.OP_XH_EXP, arg).reshape(pet.shape), 'decay')
    r_aet, r_q, r_sav = M.oracle_march(pars, pet, pr, tn, sm0, gw0, decay=decay, gw_reciprocal=fastq)
    for name, got, want in (('aet', aet, r_aet), ('q', q, r_q), ('sav', sav, r_sav)):
        for k, kind in enumerate(M.FORCINGS):
            sel = lab == k
            assert_bits(got[sel], want[sel], '{} under {}'.format(name, kind))
    nan_rows = np.isnan(q).any(axis=1)
    assert not nan_rows[lab != M.FORCINGS.index('nan_precip')].any(), 'a NaN without NaN forcing'


def test_month_update_with_infinite_precipitation(probe):
    """Infinite precipitation is outside quot()'s domain (quot(inf, 1.9) is NaN where numpy carries an infinite snowpack),
    so nothing is assumed about the NaN masks: they are compared and the difference is printed.  Where the oracle is finite
    the kernel must be finite and equal in bits, and it must not be finite where the oracle is NaN.
    Observed: the masks are identical (16,819 of 30,240 values finite on both sides, no infinite output): in the month
    the snowpack turns infinite in numpy and NaN in the kernel, rain = precip - snow is inf - inf = NaN on both sides."""
    P = M.box_parameters()[:M.N_CORNERS + M.N_FACES + 200]
    pet, pr, tn = M.forcing('inf_precip', len(P), 120, 3)
    sm0, gw0 = _init(len(P))
    aet, q, sav, decay, _ = probe.march(P, pet, pr, tn, sm0, gw0)
    r_aet, r_q, r_sav = M.oracle_march(P, pet, pr, tn, sm0, gw0, decay=decay)
    for name, got, want in (('aet', aet, r_aet), ('q', q, r_q), ('sav', sav, r_sav)):
        fin = np.isfinite(want)
        only_dev, only_ref = int((np.isnan(got) & ~np.isnan(want)).sum()), int((~np.isnan(got) & np.isnan(want)).sum())
        print('{}: {} finite in the oracle; NaN on the device only {}, in the oracle only {}, oracle infinite {}'.format(
            name, int(fin.sum()), only_dev, only_ref, int(np.isinf(want).sum())))
        assert fin.sum() > 0.2 * want.size
        assert not np.isnan(got[fin]).any(), name + ': NaN on the device where the oracle is finite'
        assert_bits(got[fin], want[fin], name + ' where the oracle is finite')
        assert only_ref == 0, name + ': the kernel must not be finite where the oracle is NaN'


# =============================================================================================== part 2: the runoff kernels
def device_decay(probe, pars, pet):
    """exp(-pet / b) as the runoff kernels form it: xh_exp(quot(-pet, b, 1 / b))."""
    b = np.broadcast_to(pars[:, 1:2] * 1000, pet.shape)
    return probe.unary(M.OP_XH_EXP, probe.binary(M.OP_QUOT, -pet, b)).reshape(pet.shape)


def run_xh_abcd(ctx, pars, pet, pr, tn, basin_index, n_groups, spinup):
    """xh_abcd through the C-ABI, one parameter row per cell.  NaN tmin goes in as it is (no nan_to_num)."""
    ncell, nm = pet.shape
    d = [ctx.upload(M.f64(a)) for a in (pars, pet, pr)] + ([ctx.upload(M.f64(tn))] if tn is not None else [None])
    out = [ctx.empty((ncell, nm)) for _ in range(3)] + [ctx.empty((n_groups,)) for _ in range(2)]
    try:
        ctx.abcd(ncell, nm, spinup, n_groups, basin_index, np.arange(ncell, dtype=np.int32), ncell, d[0], d[1], d[2], d[3],
                 out[0], out[1], out[2], out[3], out[4])
        return [o.download() for o in out]
    finally:
        for a in d + out:
            if a is not None:
                a.free()


def interleaved_forcing(ncell, nm, seed):
    """Cell i gets forcing family i mod 9, so every wave of a launch holds every family (NaN, pet = 0, ... included)."""
    k = len(M.FORCINGS)
    per = (ncell + k - 1) // k
    pet, pr, tn = (np.empty((ncell, nm)) for _ in range(3))
    for j, kind in enumerate(M.FORCINGS):
        a, b, c = M.forcing(kind, per, nm, seed)
        n = len(range(j, ncell, k))
        pet[j::k], pr[j::k], tn[j::k] = a[:n], b[:n], c[:n]
    return pet, pr, tn


def cycled_parameters(ncell):
    """Corners first, then faces, random box points and today's range, repeated: cell i gets point i mod 2542."""
    P = M.box_parameters()
    return P[np.arange(ncell) % len(P)]


def check_whole_call(ctx, probe, pars, pet, pr, tn, spinup, tag):
    """One cell per basin group: the whole call -- spin-up, December means, simulation -- equals the oracle in bits."""
    n = len(pars)
    aet, q, sav, sm0, gw0 = run_xh_abcd(ctx, pars, pet, pr, tn, np.arange(n, dtype=np.int32), n, spinup)
    ref = o_abcd.ABCD(pars, pet, pr, tn, np.arange(n), pet.shape[1], spinup, decay=device_decay(probe, pars, pet))
    ref.emulate()
    assert_bits(sm0, ref.sm0, (tag, 'sm0'))
    assert_bits(gw0, ref.gw0, (tag, 'gw0'))
    assert_bits(aet, ref.actual_et.T, (tag, 'aet'))
    assert_bits(q, ref.rsim.T, (tag, 'q'))
    assert_bits(sav, ref.soil_water_storage.T, (tag, 'sav'))


SMALL_CELLS = (1, 31, 32, 33, 63, 64, 65)
# (months, spin-up): month counts whose residues mod 16 are 0, 2, 6, 8 and 14 -- k_abcd_tile shifts the row of cell c by
# (c x nmonths) mod 16 months, so with these every shift 0 .. 14 occurs next to a tile edge -- and 26, fewer than two
# tiles; spin-ups: the shortest (25), odd ones, ones that are not a multiple of the spin-up kernel's register tile of 8,
# and one equal to the series.
SMALL_SERIES = ((48, 25), (34, 27), (38, 38), (600, 121), (40, 30), (30, 29), (26, 26))


@pytest.mark.parametrize('nm,spinup', SMALL_SERIES)
@pytest.mark.parametrize('snow_on', [True, False], ids=['snow', 'nosnow'])
def test_xh_abcd_whole_call_in_bits_small_shapes(hip, probe, nm, spinup, snow_on):
    ctx = hip.get_context()
    for ncell in SMALL_CELLS:
        pars = cycled_parameters(ncell)
        pet, pr, tn = interleaved_forcing(ncell, nm, ncell)
        check_whole_call(ctx, probe, pars, pet, pr, tn if snow_on else None, spinup, (ncell, nm, spinup))


@pytest.mark.parametrize('kind', M.FORCINGS)
def test_xh_abcd_whole_call_in_bits_over_the_box(hip, probe, kind):
    """Every parameter point of the case list (corners, face centres, 2,000 box points, 500 of today's range) through
    xh_abcd with one cell per group, 120 months, spin-up 49, with snow; every forcing family."""
    P = M.box_parameters()
    pet, pr, tn = M.forcing(kind, len(P), 120, 1)
    check_whole_call(hip.get_context(), probe, P, pet, pr, tn, 49, kind)


def tile_width_counts(cu):
    """Cell counts that select each instantiation of k_abcd_tile.  xh_abcd_enqueue_sim takes the smallest of 32 / 40 / 48
    cells per wave whose grid fits the chip's wave slots in one round, slots = 2 waves x 4 SIMDs x CUs = 8 x CUs, i.e.
    ncell <= 8 x CUs x width; above 8 x CUs x 48 it falls back to 32.  On 256 CUs: 65,536 -> 32, 65,537 -> 40, 81,921 -> 48,
    98,305 -> 32 again.  The timing record names every width "abcd_sim", so the selection is asserted by this derivation
    (and each count is checked against it below), not read back."""
    slots = 8 * cu
    def width(n):
        for c in (32, 40, 48):
            if (n + c - 1) // c <= slots:
                return c
        return 32
    counts = {slots * 32: 32, slots * 32 + 1: 40, slots * 40 + 1: 48, slots * 48 + 1: 32}
    for n, w in counts.items():
        assert width(n) == w
    return counts


# (which count, months, spin-up): every width with a month count of residue 0 and one or two with shifted rows
BIG_SHAPES = ((0, 48, 25), (1, 34, 27), (1, 30, 30), (2, 38, 25), (2, 40, 33), (3, 26, 26))


@pytest.mark.parametrize('which,nm,spinup', BIG_SHAPES)
def test_xh_abcd_tile_widths_in_bits(hip, probe, which, nm, spinup):
    """The 32-, 40- and 48-cell instantiations of k_abcd_tile and the fall back to 32 above 8 x CUs x 48 cells, with the
    last wave partly empty, many cells per basin: the returned sm0 / gw0 are injected into the oracle and the simulation
    compared in bits; the basin means themselves keep the stage bar (their sums run in another order)."""
    ctx = hip.get_context()
    counts = tile_width_counts(ctx.cu_count())
    ncell = sorted(counts)[which]
    n_groups = 37
    bidx = (np.arange(ncell) % n_groups).astype(np.int32)
    pars = cycled_parameters(ncell)
    pet, pr, tn = interleaved_forcing(ncell, nm, which)
    aet, q, sav, sm0, gw0 = run_xh_abcd(ctx, pars, pet, pr, tn, bidx, n_groups, spinup)
    decay = device_decay(probe, pars, pet)
    ref = o_abcd.ABCD(pars, pet, pr, tn, bidx, nm, spinup, decay=decay, state0=(sm0[bidx], gw0[bidx]))
    ref.emulate()
    tag = '{} cells ({} per wave), {} months'.format(ncell, counts[ncell], nm)
    assert_bits(aet, ref.actual_et.T, tag + ' aet')
    assert_bits(q, ref.rsim.T, tag + ' q')
    assert_bits(sav, ref.soil_water_storage.T, tag + ' sav')
    own = o_abcd.ABCD(pars, pet, pr, tn, bidx, nm, spinup, decay=decay)
    own.emulate()
    first = np.array([np.flatnonzero(bidx == g)[0] for g in range(n_groups)])
    for got, want in ((sm0, own.sm0[first]), (gw0, own.gw0[first])):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want) + 1e-9)


def test_xh_abcd_refuses_an_odd_month_count(hip, probe):
    ctx = hip.get_context()
    pars = cycled_parameters(4)
    pet, pr, tn = interleaved_forcing(4, 37, 0)
    with pytest.raises(hip.HipError, match='nmonths must be positive and even'):
        run_xh_abcd(ctx, pars, pet, pr, tn, np.zeros(4, dtype=np.int32), 1, 25)


@pytest.mark.parametrize('nm,block', [(120, 48), (72, 48), (192, 96)])
def test_blocked_march_equals_whole_series_at_box_corners(hip, nm, block):
    """The block pipeline's ABCD calls (m_begin > 0, the state carried in d_state) against the whole-series call, in bits,
    with box-corner parameters: block edges at 48 and 96 (multiples of 16) and the last edge at 120 or 72 (not one)."""
    from xanthos_amd import synth
    from xanthos_amd.pipeline import pipeline_from_world
    ctx = hip.get_context()
    w = synth.make_world(nrow=40, ncol=80, ncell=1500, n_basins=16, seed=12)
    corners = M.box_parameters()[:M.N_CORNERS]
    w.abcd_pars = corners[[1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31]].copy()     # m at its upper bound
    w.abcd_pars[::2, 4] = M.BOX_LO[4]
    pipe = pipeline_from_world(ctx, w, nm, 1971, 25, 0)
    ctx.synth_forcing(29, w.ncell, nm, ctx.upload(w.latitude), pipe.alloc_forcing(), nan_frac=0.002)
    names = ('pet', 'aet', 'q', 'sav')
    pipe.run(('pm', 'abcd'), fused=False, fed=False)
    ref = pipe.download(names)
    assert np.isfinite(ref['q']).sum() > 0.5 * ref['q'].size
    for k in names:
        pipe.out[k].zero()
    pipe.run_fused(with_routing=False, block_months=block)
    got = pipe.download(names)
    for k in names:
        assert_bits(got[k], ref[k], (k, nm, block))


# =============================================================================================== part 2: the calibration objective
def calib_members(n):
    """Corners and face centres of the box first (42), then random box points."""
    return M.box_parameters()[:n]


@pytest.mark.parametrize('nmem', [42, 64], ids=['cell_lanes', 'member_lanes'])
@pytest.mark.parametrize('snow_on', [True, False], ids=['snow', 'nosnow'])
def test_calibration_series_in_bits_for_one_cell(hip, probe, snow_on, nmem):
    """xh_calib_objective(want_series) for a basin of ONE cell, so that the sum over cells is the cell: the series must be
    the oracle's runoff in bits once decay is injected.  42 members run the cell-lane kernel, whose month is the runoff
    kernels' (quot() for the exp argument and the groundwater quotient): the plain oracle.  64 members run the member-lane
    kernel (exp argument -pet * (1 / b), groundwater as a product with 1 / (d + 1)): the oracle with gw_reciprocal and the
    probe's FASTQ decay.  nansum turns a NaN month into 0."""
    ctx = hip.get_context()
    nm, spinup = 120, 37
    mem = calib_members(nmem)
    pet, pr, tn = M.forcing('wet30', 1, nm, 11)
    tn = tn if snow_on else None
    npar = 5 if snow_on else 4
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a.T))
    d = [up(pet), up(pr), up(tn)]
    obs = np.linspace(10.0, 50.0, nm)
    try:
        ed, series = ctx.calib_objective(1, nm, spinup, mem[:, :npar], d[0], d[1], d[2], None, obs, want_series=True)
    finally:
        for a in d:
            if a is not None:
                a.free()
    fast = nmem >= 48
    rep = lambda a: None if a is None else np.repeat(a, nmem, axis=0)
    b = mem[:, 1:2] * 1000
    if fast:
        decay = probe.unary(M.OP_XH_EXP, (-rep(pet)) * (1.0 / b)).reshape(nmem, nm)
    else:
        decay = device_decay(probe, mem, rep(pet))
    ref = o_abcd.ABCD(mem, rep(pet), rep(pr), rep(tn), np.arange(nmem), nm, spinup, decay=decay, gw_reciprocal=fast)
    ref.emulate()
    want = np.nan_to_num(ref.rsim.T, nan=0.0) + 0.0
    assert_bits(series + 0.0, want, 'calibration series, {} members'.format(nmem))


@pytest.mark.parametrize('nmem', [42, 64], ids=['cell_lanes', 'member_lanes'])
def test_calibration_objective_at_box_corners(hip, nmem):
    """ED = 1 - KGE of a 150-cell basin at the corners and face centres of the box against oracle/calib.py, at the
    objective's own bar (1e-9): the marches use the FASTQ form and the sums over cells run in another order, so this one
    is not a comparison in bits."""
    from oracle import calib as o_calib
    ctx = hip.get_context()
    nm, spinup, ncell = 120, 25, 150
    mem = calib_members(nmem)
    pet, pr, tn = M.forcing('wet30', ncell, nm, 13)
    area = np.random.default_rng(5).uniform(500.0, 3000.0, ncell)
    obs = np.random.default_rng(6).gamma(2.0, 20.0, nm)
    up = lambda a: ctx.upload(np.ascontiguousarray(a.T))
    d = [up(pet), up(pr), up(tn), ctx.upload(area)]
    try:
        ed, series = ctx.calib_objective(ncell, nm, spinup, mem, d[0], d[1], d[2], d[3], obs, want_series=True)
    finally:
        for a in d:
            a.free()
    r_series = np.array([o_calib.basin_runoff(p, 0, pet, pr, tn, nm, spinup, 'km3_per_mth', area) for p in mem])
    r_ed = np.array([o_calib.kge_distance(s, obs) for s in r_series])
    worst_s = float(np.max(np.abs(series - r_series) / (1e-9 * np.abs(r_series) + 1e-12)))
    worst_e = float(np.max(np.abs(ed - r_ed) / (1e-9 * np.abs(r_ed) + 1e-12)))
    print('calibration at the box corners, {} members: series {:.3e} of the bar, ED {:.3e} of the bar'.format(nmem, worst_s, worst_e))
    assert np.isfinite(r_ed).all() and np.isfinite(ed).all()
    assert worst_s <= 1.0 and worst_e <= 1.0
    # xh_calib_objective_multi: the same basin beside a second one, each with the population -- same bits for the first,
    # the same bar for the second
    n2 = 70
    pet2, pr2, tn2 = M.forcing('wet15', n2, nm, 14)
    area2 = area[:n2] * 1.5
    d = [up(pet), up(pr), up(tn), ctx.upload(area), up(pet2), up(pr2), up(tn2), ctx.upload(area2)]
    try:
        ed_m, series_m = ctx.calib_objective_multi([ncell, n2], nm, spinup, np.stack([mem, mem]), [d[0], d[4]], [d[1], d[5]],
                                                   [d[2], d[6]], [d[3], d[7]], np.stack([obs, obs]), want_series=True)
    finally:
        for a in d:
            a.free()
    assert_bits(ed_m[0], ed, 'ED of the first basin of a two-basin call')
    assert_bits(series_m[0], series, 'series of the first basin of a two-basin call')
    r2 = np.array([o_calib.basin_runoff(p, 0, pet2, pr2, tn2, nm, spinup, 'km3_per_mth', area2) for p in mem])
    r2_ed = np.array([o_calib.kge_distance(s, obs) for s in r2])
    worst_s = float(np.max(np.abs(series_m[1] - r2) / (1e-9 * np.abs(r2) + 1e-12)))
    worst_e = float(np.max(np.abs(ed_m[1] - r2_ed) / (1e-9 * np.abs(r2_ed) + 1e-12)))
    print('  second basin of the two-basin call: series {:.3e} of the bar, ED {:.3e} of the bar'.format(worst_s, worst_e))
    assert worst_s <= 1.0 and worst_e <= 1.0
