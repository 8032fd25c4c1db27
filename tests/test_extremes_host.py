"""Annual extremes, L-moments and the GEV per row, everything a machine without a GPU can check: the numpy
restatement (tests/extremes_np.py) against scipy.stats.lmoment and scipy.stats.genextreme, the host build of
csrc/xh_extremes_dev.h (tests/extremes_probe) against the restatement, both against 40-digit values, the annual reduction,
the counted sort and the sums against std::sort under the sanitizers, the [Extremes] section's refusals and the C-ABI
bookkeeping.

What is bit for bit and what is bounded.  n, the annual series, l1, l2, t3 and t4 are comparisons and +, -, x, / in a fixed
order: the restatement, the host build and the device give the same bits.  k, alpha, xi, the return levels and T_y pass
through expm1, log1p, exp, log and Gamma, which every build takes from another library, and they inherit the rounding of the
sums: tests/golden/make_golden_extremes.py measures, in the measures of tests/extremes_cases.errors, how far the restatement
lies from 40-digit values on 300 rows a year count and kind, per row class:

    quantity    ordinary     shifted by 1e6 (2 b1 - b0 cancels)
    lmom        1.755e-13    9.921e-10
    k           1.118e-12    8.552e-09
    alpha       1.159e-13    5.264e-10
    xi          7.219e-15    3.143e-15
    level       9.734e-14    6.926e-14
    T_year      8.282e-11    1.178e-07      (the largest year of a row lies near the end of the fitted support)
    sweep       k 4.103e-14, alpha 2.665e-15, xi 1.326e-15   (the pieces over t3, no sums)
    scipy.stats.lmoment's own error: 9.814e-14 / 7.876e-10

The bound on every implementation is 4 x the figure of its quantity and class (the margin because the device's exp, log and
Gamma are other implementations), and not below 4 ulp.  k is held absolutely below |k| = 2^-5 (as a relative error at 2^-5)
and relatively above.  alpha is held against the larger of alpha and l2: towards k = -1 alpha falls to 0 like 1 + k, and
Gamma(1 + k) turns the last bits of k into a RELATIVE error of alpha of eps / (1 + k) in every implementation (a run's cell
with t3 = 0.9992, k = -0.9993: device and restatement 6.1e-13 apart relative to alpha, 5e-16 relative to l2)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import extremes_cases as cases
import extremes_np
from xanthos_amd import ConfigReader, ValidationException, _hip, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PROBE_DIR = os.path.join(ROOT, 'tests', 'extremes_probe')
P = ctypes.c_void_p
EPS = cases.EPS
MEASURED = {('lmom', 'ordinary'): 1.755e-13, ('lmom', 'shifted'): 9.921e-10, ('k', 'ordinary'): 1.118e-12, ('k', 'shifted'): 8.552e-09,
            ('alpha', 'ordinary'): 1.159e-13, ('alpha', 'shifted'): 5.264e-10, ('xi', 'ordinary'): 7.219e-15,
            ('xi', 'shifted'): 3.143e-15, ('level', 'ordinary'): 9.734e-14, ('level', 'shifted'): 6.926e-14,
            ('T_year', 'ordinary'): 8.282e-11, ('T_year', 'shifted'): 1.178e-07}
MEASURED_SWEEP = {'k': 4.103e-14, 'alpha': 2.665e-15, 'xi': 1.326e-15}
MEASURED_SCIPY = {'ordinary': 9.814e-14, 'shifted': 7.876e-10}


def bound(golden, quantity, cls):
    measured = float(golden('extremes')['np_err_{}_{}'.format(quantity, cls)])
    assert measured == pytest.approx(MEASURED[(quantity, cls)], rel=1e-3)         # the figure of the docstring
    return max(4.0 * measured, 4.0 * EPS)


def sweep_bound(golden, name):
    measured = float(golden('extremes')['np_err_sweep_' + name])
    assert measured == pytest.approx(MEASURED_SWEEP[name], rel=1e-3)
    return max(4.0 * measured, 4.0 * EPS)


def within(golden, got, ref, tag, quantities=cases.QUANTITIES, classes=None):
    """(table, annual, T_year) against the reference's: the masks, and every quantity of every row inside its class' bound.
    ``classes``: the class of every row, or one name for all; None: the rows are those of extremes_cases.make_rows."""
    assert cases.same_masks(got[0], got[1], got[2], ref[0], ref[1], ref[2]), tag
    err = cases.errors(got[0], got[2], ref[0], ref[2])
    nrows = got[0].shape[0]
    cls = np.array([cases.class_of(r) for r in range(nrows)]) if classes is None else np.broadcast_to(np.asarray(classes), (nrows,))
    for q in quantities:
        for c in cases.CLASSES:
            e = err[q][(cls == c) & ~np.isnan(err[q])]
            worst, b = (float(e.max()) if e.size else 0.0), bound(golden, q, c)
            print('{}: {} ({}) max error {:.3e}, bound {:.3e}'.format(tag, q, c, worst, b))
            assert worst <= b, (tag, q, c, worst, b)


@pytest.fixture(scope='module')
def probe():
    """tests/extremes_probe/libextremes_probe.so and series_check (build() makes them; made here when the suite runs without
    it)."""
    path = os.path.join(PROBE_DIR, 'libextremes_probe.so')
    if not os.path.isfile(path) or not os.path.isfile(os.path.join(PROBE_DIR, 'series_check')):
        subprocess.run(['make', '-C', PROBE_DIR], check=True, capture_output=True)
    lib = ctypes.CDLL(path)
    lib.ep_extremes.restype = ctypes.c_int
    lib.ep_extremes.argtypes = [ctypes.c_int64] + [ctypes.c_int32] * 6 + [P] * 6
    for name, nargs in (('ep_k_of_t3', 2), ('ep_parameters', 5), ('ep_quantile', 5), ('ep_cdf', 5), ('ep_return_period', 5)):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [ctypes.c_int64] + [P] * nargs
    return lib


def host_extremes(probe, rows, kind, T=cases.GOLDEN_T, min_years=cases.MIN_YEARS, start=0, nyear=None, parameters=None,
                  annual=True, T_year=True, fill=-777.0):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    nyear = (rows.shape[1] - start) // 12 if nyear is None else nyear
    T = np.ascontiguousarray(T, dtype=np.float64)
    table = np.full((rows.shape[0], 8 + T.size), fill)
    a, ty = np.full((rows.shape[0], nyear), fill), np.full((rows.shape[0], nyear), fill)
    par = None if parameters is None else np.ascontiguousarray(np.asarray(parameters)[:, :8], dtype=np.float64)
    rc = probe.ep_extremes(rows.shape[0], rows.shape[1], start, nyear, extremes_np.KINDS.index(kind), min_years, T.size,
                           T.ctypes.data_as(P), rows.ctypes.data_as(P), None if par is None else par.ctypes.data_as(P),
                           table.ctypes.data_as(P), a.ctypes.data_as(P) if annual else None, ty.ctypes.data_as(P) if T_year else None)
    assert rc == 0
    return table, a, ty


def piece(probe, name, *arrays):
    arrays = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), np.broadcast(*arrays).shape)) for a in arrays]
    outs = [np.full(arrays[0].shape, -777.0) for _ in range(2 if name == 'ep_parameters' else 1)]
    getattr(probe, name)(arrays[0].size, *[a.ctypes.data_as(P) for a in arrays + outs])
    return outs if len(outs) > 1 else outs[0]


@pytest.fixture(scope='module')
def reference():
    """The restatement of the host rows of every year count and kind, computed once."""
    return {(ny, kind): extremes_np.extremes_rows(cases.make_rows(ny, cases.HOST_ROWS), kind, cases.GOLDEN_T, min_years=cases.MIN_YEARS)
            for ny in cases.YEARS for kind in extremes_np.KINDS}


def test_the_rows_cover_what_they_should(reference):
    kinds = [cases.kind_of(r) for r in range(cases.HOST_ROWS)]
    assert set(kinds) == set(cases.KINDS) and cases.YEARS == (5, 10, 50, 63, 64, 65, 129, 341)
    for (ny, kind), (table, annual, T_year) in reference.items():
        fit = ~np.isnan(table[:, 5])
        by = {k: [r for r in range(cases.HOST_ROWS) if kinds[r] == k] for k in cases.KINDS}
        assert not fit[by['constant']].any() and not fit[by['all_nan']].any() and not fit[by['few']].any()
        assert (table[by['all_nan'], 0] == 0).all() and (table[by['few'], 0] < cases.MIN_YEARS).all()
        assert (table[by['year_nan'], 0] == ny - 1).all() and np.isnan(table[by['all_nan'], 1:]).all()
        assert not np.isnan(table[by['constant'], :3]).any() and np.isnan(table[by['constant'], 3:]).all()
        if ny >= 50:
            assert fit[[r for k in cases.KINDS if k.startswith('gev') or k in ('shifted', 'negative') for r in by[k]]].all()
    ks = np.concatenate([t[0][:, 5] for t in reference.values()])
    assert np.nanmin(ks) < -0.4 and np.nanmax(ks) > 0.6 and (np.abs(ks[~np.isnan(ks)]) < 0.25).any()


# ------------------------------------------------------------------ (1) the restatement against scipy
def test_restatement_against_scipy_lmoment_and_genextreme(reference, golden):
    from scipy import stats
    g = golden('extremes')
    checked = 0
    for (ny, kind), (table, annual, T_year) in reference.items():
        sign = -1.0 if kind == 'min' else 1.0
        for r in np.flatnonzero(~np.isnan(table[:, 5])):
            cls = cases.class_of(r)
            own, scipys = float(g['np_err_lmom_' + cls]), float(g['scipy_err_lmom_' + cls])
            assert own == pytest.approx(MEASURED[('lmom', cls)], rel=1e-3) and scipys == pytest.approx(MEASURED_SCIPY[cls], rel=1e-3)
            z = sign * annual[r][~np.isnan(annual[r])]
            lm = np.array(stats.lmoment(z, order=[1, 2, 3, 4], standardize=True))
            mine = table[r, 1:5] * [sign, 1.0, 1.0, 1.0]
            # two summations of the same numbers: each within its own measured error of the 40-digit value, 4 x the sum
            assert cases.lmom_error(mine[None, :], lm[None, :])[0] <= 4.0 * (own + scipys), (ny, kind, r)
            k, alpha, xi = table[r, 5], table[r, 6], sign * table[r, 7]
            ppf = stats.genextreme.ppf(1.0 - 1.0 / np.array(cases.GOLDEN_T), k, loc=xi, scale=alpha)
            scale = max(abs(table[r, 1]), table[r, 2])
            err = np.abs(sign * table[r, 8:] - ppf) / np.maximum(np.abs(ppf), scale)
            assert (err <= bound(golden, 'level', cls)).all(), (ny, kind, r, err)
            checked += 1
    assert checked > 300


# ------------------------------------------------------------------ (2) the host build of the header
@pytest.mark.parametrize('kind', extremes_np.KINDS)
@pytest.mark.parametrize('years', cases.YEARS)
def test_host_build_of_the_header_against_the_restatement(probe, reference, golden, years, kind):
    got = host_extremes(probe, cases.make_rows(years, cases.HOST_ROWS), kind)
    ref = reference[(years, kind)]
    assert cases.bits_equal(got[0], got[1], ref[0], ref[1]), np.argwhere(got[0][:, :5] != ref[0][:, :5])
    within(golden, got, ref, 'host {} {}'.format(years, kind))


def test_window_inside_a_longer_row_and_other_periods(probe, golden):
    wide = cases.make_rows(30, cases.HOST_ROWS)
    wide = np.concatenate([wide[:, -7:], wide, wide[:, :10]], axis=1)
    for start, nyear, T in ((0, 30, (2.0,)), (7, 30, (1.5, 2, 5, 10, 20, 50, 100, 500)), (17, 29, ()), (9, 12, (10.0, 3.0))):
        for kind in extremes_np.KINDS:
            got = host_extremes(probe, wide, kind, T=T, start=start, nyear=nyear)
            ref = extremes_np.extremes_rows(wide, kind, T, min_years=cases.MIN_YEARS, start=start, nyear=nyear)
            assert got[0].shape == (cases.HOST_ROWS, 8 + len(T)) and cases.bits_equal(got[0], got[1], ref[0], ref[1])
            within(golden, got, ref, 'window {} {} {}'.format(start, nyear, kind))
    # min_years decides the fit, not the sums
    a = host_extremes(probe, wide, 'max', start=7, nyear=12, min_years=12)
    b = host_extremes(probe, wide, 'max', start=7, nyear=12, min_years=13)
    assert np.isnan(b[0][:, 3:]).all() and np.isnan(b[2]).all() and a[0][:, :3].tobytes() == b[0][:, :3].tobytes()
    assert (~np.isnan(a[0][:, 5])).sum() > cases.HOST_ROWS // 2


def test_probe_refuses_what_the_entry_refuses(probe):
    x = np.zeros((2, 130))
    T = np.array([2.0, 10.0])
    table, a = np.full((2, 10), -777.0), np.full((2, 10), -777.0)

    def call(stride=130, col0=0, nyear=10, kind=0, min_years=5, nT=2, T=T, x=x, table=table):
        return probe.ep_extremes(2, stride, col0, nyear, kind, min_years, nT, None if T is None else T.ctypes.data_as(P),
                                 None if x is None else x.ctypes.data_as(P), None, None if table is None else table.ctypes.data_as(P),
                                 a.ctypes.data_as(P), None)
    for bad in (dict(x=None), dict(table=None), dict(T=None), dict(col0=-1), dict(col0=11), dict(nyear=0), dict(nyear=11),
                dict(stride=5000, nyear=342), dict(nT=-1), dict(nT=9), dict(T=np.array([2.0, 1.0])), dict(T=np.array([np.nan, 3.0])),
                dict(kind=2), dict(kind=-1), dict(min_years=4)):
        assert call(**bad) == 1, bad
    assert (table == -777.0).all() and (a == -777.0).all()
    assert call() == 0 and call(col0=10) == 0 and call(nT=0, T=None) == 0


# ------------------------------------------------------------------ (3) 40 digits
@pytest.mark.parametrize('kind', extremes_np.KINDS)
@pytest.mark.parametrize('years', cases.YEARS)
def test_restatement_and_host_build_against_40_digits(probe, reference, golden, years, kind):
    g = golden('extremes')
    ref = (g['table_{}_{}'.format(kind, years)], reference[(years, kind)][1], g['T_year_{}_{}'.format(kind, years)])
    assert ref[0].shape == (cases.HOST_ROWS, 12) and ref[2].shape == (cases.HOST_ROWS, years)
    within(golden, reference[(years, kind)], ref, 'restatement {} {}'.format(years, kind))
    within(golden, host_extremes(probe, cases.make_rows(years, cases.HOST_ROWS), kind), ref, 'host {} {}'.format(years, kind))


def test_the_pieces_over_the_t3_sweep_against_40_digits(probe, golden):
    g = golden('extremes')
    t3, gk, ga, gx = g['sweep_t3'], g['sweep_k'], g['sweep_alpha'], g['sweep_xi']
    # the sweep puts k at 0 (to the rounding of t3), +-1e-12, +-1e-8, +-1e-5, +-1e-3, on both sides of both switch-overs,
    # and t3 at +-0.95 and 0.99
    for want in (1e-12, 1e-8, 1e-5, 1e-3):
        assert (np.abs(np.abs(gk) / want - 1.0) < 1e-3).sum() == 2
    assert (np.abs(gk) < 1e-15).sum() == 1 and t3.min() == -0.95 and t3.max() == 0.99
    for edge in (extremes_np.K_DLOG_SERIES, extremes_np.K_SERIES):
        near = np.abs(np.abs(gk) / edge - 1.0) < 2e-3
        assert (near & (np.abs(gk) < edge)).sum() == 2 and (near & (np.abs(gk) > edge)).sum() == 2
    one, zero = np.ones(t3.size), np.zeros(t3.size)
    for name, k in (('restatement', extremes_np.k_of_t3(t3)), ('host', piece(probe, 'ep_k_of_t3', t3))):
        alpha, xi = extremes_np.gev_parameters(zero, one, k) if name == 'restatement' else piece(probe, 'ep_parameters', zero, one, k)
        err = cases.sweep_errors(k, alpha, xi, gk, ga, gx)
        for q in ('k', 'alpha', 'xi'):
            print('{}: sweep {} max error {:.3e}, bound {:.3e}'.format(name, q, float(err[q].max()), sweep_bound(golden, q)))
            assert (err[q] <= sweep_bound(golden, q)).all(), (name, q, t3[np.argmax(err[q])])
    # the Gumbel limit itself
    alpha, xi = piece(probe, 'ep_parameters', 0.0, 1.0, 0.0)
    assert abs(alpha[()] - 1.0 / np.log(2.0)) <= 2 * EPS and abs(xi[()] + np.euler_gamma / np.log(2.0)) <= 2 * EPS


def test_quantile_cdf_and_return_period_agree(probe):
    rng = np.random.default_rng(3)
    k = np.concatenate([rng.uniform(-0.9, 1.5, 400), [0.0, 1e-12, -1e-12, 1e-5, -1e-5]])
    alpha, xi = rng.uniform(0.5, 20.0, k.size), rng.uniform(-50.0, 50.0, k.size)
    for T in (1.01, 2.0, 10.0, 100.0, 1000.0):
        q = piece(probe, 'ep_quantile', np.full(k.size, T), k, alpha, xi)
        assert np.allclose(q, extremes_np.quantile(T, k, alpha, xi), rtol=1e-12, atol=1e-12)
        F = piece(probe, 'ep_cdf', q, k, alpha, xi)
        assert np.allclose(F, 1.0 - 1.0 / T, rtol=0, atol=1e-12 * T)
        back = piece(probe, 'ep_return_period', q, k, alpha, xi)
        assert np.allclose(back, T, rtol=1e-9 * T)
        assert np.allclose(back, extremes_np.return_period(q, k, alpha, xi), rtol=1e-9 * T)
    # outside the support: above the upper bound of k > 0 F = 1 and T = inf, below the lower bound of k < 0 F = 0 and T = 1
    above = piece(probe, 'ep_return_period', 1e9, 0.5, 2.0, 1.0), piece(probe, 'ep_cdf', 1e9, 0.5, 2.0, 1.0)
    below = piece(probe, 'ep_return_period', -1e9, -0.5, 2.0, 1.0), piece(probe, 'ep_cdf', -1e9, -0.5, 2.0, 1.0)
    assert above[0][()] == np.inf and above[1][()] == 1.0 and below[0][()] == 1.0 and below[1][()] == 0.0
    assert np.isnan(piece(probe, 'ep_return_period', np.nan, 0.1, 2.0, 1.0)[()])
    assert np.isnan(piece(probe, 'ep_return_period', 1.0, np.nan, np.nan, np.nan)[()])


# ------------------------------------------------------------------ (4) min is max of the negated row
@pytest.mark.parametrize('years', cases.YEARS)
def test_min_is_max_of_the_negated_row_bit_for_bit(probe, years):
    rows = cases.make_rows(years, cases.HOST_ROWS)
    for f in (lambda r, kind: host_extremes(probe, r, kind), lambda r, kind: extremes_np.extremes_rows(r, kind, cases.GOLDEN_T, cases.MIN_YEARS)):
        lo, hi = f(rows, 'min'), f(-rows, 'max')
        flip = np.ones(12)
        flip[[1, 7, 8, 9, 10, 11]] = -1.0                      # l1, xi and the return levels
        assert lo[0].tobytes() == (hi[0] * flip).tobytes() or np.array_equal(lo[0], hi[0] * flip, equal_nan=True)
        assert np.array_equal(lo[1], -hi[1], equal_nan=True) and np.array_equal(lo[2], hi[2], equal_nan=True)
        assert (~np.isnan(lo[0][:, 5])).any()


# ------------------------------------------------------------------ (5) parameters handed in
def test_parameters_handed_in_are_copied_and_used(probe, golden):
    hist = cases.make_rows(50, cases.HOST_ROWS)
    future = cases.make_rows(10, cases.HOST_ROWS, seed=7) * 1.2
    for kind in extremes_np.KINDS:
        table = host_extremes(probe, hist, kind)[0]                                   # [rows, 12]: more than 8 columns
        got = host_extremes(probe, future, kind, T=(10.0, 100.0), parameters=table)
        assert got[0][:, :8].tobytes() == table[:, :8].tobytes()
        assert np.array_equal(got[0][:, 8:], table[:, [9, 10]], equal_nan=True) or np.allclose(got[0][:, 8:], table[:, [9, 10]], rtol=1e-15, equal_nan=True)
        ref = extremes_np.extremes_rows(future, kind, (10.0, 100.0), parameters=table)
        assert ref[0][:, :8].tobytes() == table[:, :8].tobytes() and got[1].tobytes() == ref[1].tobytes()
        within(golden, got, ref, 'parameters ' + kind, quantities=('level', 'T_year'))
        fit = ~np.isnan(table[:, 5])
        ok = ~np.isnan(got[1])
        assert np.array_equal(np.isnan(got[2]), ~(ok & fit[:, None])) and (got[2][ok & fit[:, None]] >= 1.0).all()
        # the future is wetter: under the historic fit its years are rarer than under its own
        own = host_extremes(probe, future, kind, T=(10.0, 100.0))
        assert not np.array_equal(own[2], got[2], equal_nan=True)


# ------------------------------------------------------------------ (6) the series under the sanitizers
def test_annual_reduction_sort_and_sums_under_sanitizers(probe):
    """xh_ex_annual, xh_ex_rank, xh_ex_pwm and xh_extremes_row in a stand-alone program of their own
    (tests/extremes_probe/series_check.cpp, -fsanitize=address,undefined), started as a child process: rows with ties, signed
    zeros, NaN and infinite months and missing years at 1 .. 8, 63, 64, 65, 128, 129 and 341 years and random counts, teams of
    1, 3 and 64 lanes, in buffers of exactly the sizes the kernel gives a wavefront, against std::stable_sort and plain loops."""
    out = subprocess.run([os.path.join(PROBE_DIR, 'series_check'), '400', '20262'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and '400 cases, 0 failed' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ------------------------------------------------------------------ (7) the section
NM = 144


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('extremes_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = synth.make_forcing(w, NM, seed=50)
    plain = synth.write_example(root, w, f, 1971, 1982, runoff_spinup=25, routing_spinup=6)
    ini = synth.write_example(root, w, f, 1971, 1982, runoff_spinup=25, routing_spinup=6, project='with_extremes')
    synth.enable_extremes(ini, extreme_vars=('q', 'avgchflow'), kinds=('max', 'min'))
    return root, w, f, plain, ini


def edited(ini, tmp_path, *subs, name='edited.ini'):
    text = open(ini).read()
    for pattern, repl in subs:
        text, n = re.subn(pattern, repl, text)
        assert n >= 1, pattern
    path = str(tmp_path / name)
    open(path, 'w').write(text)
    return path


def refused(ini, *keys):
    with pytest.raises(ValidationException) as exc:
        ConfigReader(ini)
    msg = str(exc.value)
    assert '[Extremes]' in msg and all(k in msg for k in keys), msg
    return msg


KINDS_LINE = r'kinds = max, min'


def test_section_and_its_defaults(tree, tmp_path):
    root, w, f, plain, ini = tree
    from xanthos_amd import extremes
    c = ConfigReader(ini)
    assert c.CalculateExtremes == 1
    assert c.extremes == {'vars': ['q', 'avgchflow'], 'kinds': ['max', 'min'], 'return_periods': [2.0, 5.0, 10.0, 20.0, 50.0, 100.0],
                          'start_year': 1971, 'end_year': 1982, 'year_start_month': 1, 'min_years': 10, 'parameters': None}
    c = ConfigReader(edited(ini, tmp_path, (r'extreme_vars = q, avgchflow', 'extreme_vars = PET, aet, soilmoisture, precip'),
                            (KINDS_LINE, 'kinds = Min\nreturn_periods = 1.5, 30\nyear_start_month = 10\nmin_years = 5\nstart_year = 1972')))
    assert c.extremes['vars'] == ['pet', 'aet', 'soilmoisture', 'precip'] and c.extremes['kinds'] == ['min']
    assert c.extremes['return_periods'] == [1.5, 30.0] and c.extremes['year_start_month'] == 10 and c.extremes['min_years'] == 5
    # the hydrological year that starts in October 1981 is the last that ends inside 1982
    assert (c.extremes['start_year'], c.extremes['end_year']) == (1972, 1981)
    assert os.path.basename(extremes.output_stem(c, 'q', 'max')) == 'extremes_q_max_with_extremes'
    assert os.path.basename(extremes.output_stem(c, 'q', 'min', 'return_period')) == 'extremes_q_min_return_period_with_extremes'
    assert extremes.COLUMNS == extremes_np.COLUMNS and extremes.KINDS == extremes_np.KINDS and len(extremes.COLUMNS) == 8
    base = vars(ConfigReader(plain))
    assert base['CalculateExtremes'] == 0 and base['extremes'] is None and 'Extremes' not in open(plain).read()


def test_enable_extremes_writes_the_section(tree, tmp_path):
    root, w, f, plain, ini = tree
    path = edited(plain, tmp_path, (r'$^', ''), name='enabled.ini') if False else str(tmp_path / 'enabled.ini')
    open(path, 'w').write(open(plain).read())
    assert synth.enable_extremes(path, extreme_vars=('q',), kinds=('min',), return_periods=(2, 10), year_start_month=4, min_years=6,
                                 start_year=1973) == path
    text = open(path).read()
    assert 'CalculateExtremes = 1' in text.split('[PET]')[0] and text.rstrip().endswith('start_year = 1973')
    assert '[Extremes]\nextreme_vars = q\nkinds = min\nreturn_periods = 2, 10\nyear_start_month = 4\nmin_years = 6' in text
    c = ConfigReader(path)
    assert c.extremes['return_periods'] == [2.0, 10.0] and (c.extremes['start_year'], c.extremes['end_year']) == (1973, 1981)


def test_refusals_name_their_key(tree, tmp_path):
    root, w, f, plain, ini = tree
    refused(edited(ini, tmp_path, (r'extreme_vars = q, avgchflow', 'extreme_vars = q, chstorage')), 'extreme_vars', 'chstorage')
    refused(edited(ini, tmp_path, (r'extreme_vars = q, avgchflow', 'extreme_vars = q, q')), 'extreme_vars')
    refused(edited(ini, tmp_path, (r'extreme_vars = q, avgchflow\n', '')), 'extreme_vars')
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, mean')), 'kinds', 'mean')
    refused(edited(ini, tmp_path, (KINDS_LINE + r'\n', '')), 'kinds')
    # avgchflow without routing
    msg = refused(edited(ini, tmp_path, (r'(?s)\[Routing\].*?\n\[Extremes\]', '[Extremes]')), 'extreme_vars', 'avgchflow')
    assert 'routing_module' in msg
    # precip (and q) without a runoff module
    no_runoff = ((r'(?s)\[Runoff\].*?\n\[Routing\]', '[Routing]'), (r'(?s)\[Routing\].*?\n\[Extremes\]', '[Extremes]'))
    for var in ('precip', 'q', 'aet', 'soilmoisture'):
        msg = refused(edited(ini, tmp_path, (r'extreme_vars = q, avgchflow', 'extreme_vars = ' + var), *no_runoff), 'extreme_vars', var)
        assert 'runoff_module' in msg
    # pet without the module that makes it: PET from a file
    pet_file = os.path.join(root, 'pet.npy')
    np.save(pet_file, np.ones((w.ncell, NM)))
    msg = refused(edited(ini, tmp_path, (r'(?s)\[PET\].*?\n\[Runoff\]', '[PET]\npet_module = none\npet_file = {}\n\n[Runoff]'.format(
        pet_file)), (r'extreme_vars = q, avgchflow', 'extreme_vars = pet')), 'extreme_vars', 'pet')
    assert 'pet_module' in msg
    # the window
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nstart_year = 1970')), 'start_year', '1970')
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nend_year = 1983')), 'end_year', '1983')
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nstart_year = soon')), 'start_year', 'soon')
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nstart_year = 1974')), 'end_year', '9 years', 'min_years = 10')
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nmin_years = 13')), 'end_year', '12 years', 'min_years = 13')
    # an incomplete last hydrological year
    msg = refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nyear_start_month = 10\nend_year = 1982')), 'end_year', '1982', 'month 10')
    assert '1981' in msg
    for bad in ('0', '13', 'october'):
        refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nyear_start_month = ' + bad)), 'year_start_month', bad)
    for bad in ('4', '0', 'many'):
        refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nmin_years = ' + bad)), 'min_years', bad)
    for bad in ('1', '0.5, 10', '10, 10', '2, 3, 4, 5, 6, 7, 8, 9, 10', 'often', 'inf', 'nan'):
        refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max\nreturn_periods = ' + bad)), 'return_periods')
    refused(edited(ini, tmp_path, (r'OutputInYear = 0', 'OutputInYear = 1')), 'OutputInYear')
    # parameters: a missing table, a table of another grid
    stem = os.path.join(root, 'historic', 'hist')
    os.makedirs(os.path.dirname(stem))
    msg = refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, min\nparameters = ' + stem)), 'parameters', 'extremes_q_max_hist.npy')
    for var in ('q', 'avgchflow'):
        for kind in ('max', 'min'):
            np.save(os.path.join(root, 'historic', 'extremes_{}_{}_hist.npy'.format(var, kind)), np.zeros((w.ncell, 14)))
    c = ConfigReader(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, min\nparameters = ' + stem)))
    assert c.extremes['parameters'][('avgchflow', 'min')] == os.path.join(root, 'historic', 'extremes_avgchflow_min_hist.npy')
    np.save(os.path.join(root, 'historic', 'extremes_avgchflow_min_hist.npy'), np.zeros((w.ncell + 1, 14)))
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, min\nparameters = ' + stem)), 'parameters', 'extremes_avgchflow_min_hist.npy', str(w.ncell))
    np.save(os.path.join(root, 'historic', 'extremes_avgchflow_min_hist.npy'), np.zeros((w.ncell, 7)))
    refused(edited(ini, tmp_path, (KINDS_LINE, 'kinds = max, min\nparameters = ' + stem)), 'parameters', 'extremes_avgchflow_min_hist.npy')
    # the flag and the section
    with pytest.raises(ValidationException, match='CalculateExtremes'):
        ConfigReader(edited(ini, tmp_path, (r'CalculateExtremes = 1', 'CalculateExtremes = yes')))
    with pytest.raises(ValidationException, match=r'CalculateExtremes = 1 but the config file has no \[Extremes\] section'):
        ConfigReader(edited(ini, tmp_path, (r'(?s)\n\[Extremes\].*$', '\n')))


def test_a_window_beyond_4096_months_is_refused(tree):
    root, w, f, plain, ini = tree
    c = ConfigReader(ini)
    c.StartYear, c.EndYear = 1700, 2041
    with pytest.raises(ValidationException) as exc:
        c.configure_extremes({'extreme_vars': 'q', 'kinds': ['max']})
    assert '[Extremes] end_year' in str(exc.value) and '4104 months' in str(exc.value) and '4096' in str(exc.value)
    c.configure_extremes({'extreme_vars': 'q', 'kinds': 'max', 'year_start_month': '10'})          # 341 years
    assert c.extremes['end_year'] == 2040


def test_calibration_and_ensembles_are_refused(tree, tmp_path):
    root, w, f, plain, ini = tree
    c = ConfigReader(ini)
    c.calibrate = 1
    with pytest.raises(ValidationException, match=r'\[Extremes\] and Calibrate = 1'):
        c.configure_extremes({'extreme_vars': 'q', 'kinds': 'max'})
    c.calibrate = 0
    c.ensemble = {'members': 'members.csv'}
    with pytest.raises(ValidationException, match=r'\[Extremes\] and an \[Ensemble\] section'):
        c.configure_extremes({'extreme_vars': 'q', 'kinds': 'max'})
    with_ens = edited(ini, tmp_path, (r'(?s)$', '\n[Ensemble]\nmembers = members.csv\n'), name='ens.ini')
    try:
        ConfigReader(with_ens)
    except ValidationException as exc:          # whichever section speaks first, the run does not start
        assert '[Extremes]' in str(exc) or '[Ensemble]' in str(exc)
    else:
        raise AssertionError('an ini with [Extremes] and [Ensemble] was accepted')
    from xanthos_amd import ensemble
    with pytest.raises(ValidationException) as exc:
        ensemble.validate(ConfigReader(ini), [('a', {})])
    assert 'CalculateExtremes' in str(exc.value) and '[Ensemble]' in str(exc.value)


# ------------------------------------------------------------------ the C-ABI entry
def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    assert re.search(r'\bint xh_extremes\(xh_ctx \*ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t kind, '
                     r'int32_t min_years,\s+int32_t nT, const double \*h_T, const double \*d_x, const double \*d_par_in, '
                     r'double \*d_table, double \*d_annual,\s+double \*d_T_year\);', header)
    assert re.search(r'#define XH_EXTREMES_NPAR 8\b', header) and 'xh_extremes replaces NO function of the reference' in header
    assert len(_hip.SIGNATURES['xh_extremes'][1]) == 14
    assert hasattr(_hip.lib(), 'xh_extremes') and _hip.lib().xh_abi_version() == _hip.ABI_VERSION == 7
    assert hasattr(_hip.Context, 'extremes') and _hip.EXTREMES_KIND == {'max': 0, 'min': 1}
    dev = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'xh_extremes_dev.h')).read()
    assert re.search(r'#define XH_EXTREMES_NPAR 8\b', dev) and '__host__ __device__' in dev
    assert re.search(r'#define XH_EX_NEWTON {}\b'.format(extremes_np.NEWTON_STEPS), dev)
    assert re.search(r'#define XH_EX_K_SERIES {}\b'.format(extremes_np.K_SERIES), dev)
    block = re.search(r'const double c\[30\] = \{(.*?)\};', dev, re.S).group(1)      # the header's series is the restatement's
    assert tuple(float(v) for v in block.replace('\n', ' ').split(',')) == extremes_np.GAMMA_TAYLOR
