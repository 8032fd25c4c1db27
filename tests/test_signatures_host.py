"""Flow duration curve and regime signatures per row, everything a machine without a GPU can check: the numpy
restatement (tests/signatures_np.py) against np.quantile, np.mean and np.std, the host build of csrc/xh_signatures_dev.h
(tests/signatures_probe) against the restatement, both against 40-digit values, the load, the sort and the order statistics
against std::sort under the sanitizers, the [Signatures] section's refusals and the C-ABI bookkeeping.

What is bit for bit and what is bounded.  Every column but two is comparisons, +, -, x, / and sqrt in a fixed order: the
restatement, the host build and the device give the same bits.  fdc_slope passes through log and centroid through atan2, which
every build takes from another library.  tests/golden/make_golden_signatures.py measures how far the restatement lies from
40-digit values over the 15 kinds of row at the 8 year counts of tests/signatures_cases.py, per quantity (relative to the 40-digit
value, absolute where that is 0):

    n, n_zero, peak_month, low_month, n_years   0
    mean          2.400e-16      std            8.883e-16      cv           3.126e-16      median       1.078e-16
    lag1          2.127e-11      flashiness     3.135e-16      regime_total 6.321e-15      seasonality  2.337e-11
    concentration 2.937e-11      annual_mean    5.521e-15      annual_cv    1.011e-10      fdc 6.957e-15, regime 6.241e-15
    fdc_slope     3.189e-15      relative to max(|slope|, 1)
    centroid      5.581e-16      the circular distance in months times the row's concentration

(the figures of 1e-11 and 1e-10 belong to the row shifted by 1e6, whose deviations cancel six digits).  The two bounded
columns are held, in every implementation and on every row, to 4 x their figure against the 40-digit value -- the margin
because the device's log and atan2 are other implementations -- and not below 4 ulp: 4 x 2^-52 for the slope's relative
measure, 4 x 2^-49 (the spacing of doubles at 12 months) for the centroid's.  The other columns of the restatement are held to
the 40-digit values by a bound from first-order error propagation, written down at `tolerances`."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import signatures_cases as cases
import signatures_np as snp
from xanthos_amd import ConfigReader, ValidationException, _hip, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PROBE_DIR = os.path.join(ROOT, 'tests', 'signatures_probe')
P = ctypes.c_void_p
EPS = 2.0 ** -52
BIT_COLUMNS = [c for c in range(snp.NCOL) if c not in (8, 13)]
MEASURED = {'fdc_slope': 3.189e-15, 'centroid': 5.581e-16}
PROBS = snp.probabilities(cases.EXCEEDANCE)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def bounded_columns(golden, table, years, tag):
    """fdc_slope and centroid of ``table`` (the rows of signatures_cases.rows(years), cal0 = CAL0) against the 40-digit values:
    every row, none left out."""
    g = golden('signatures')
    dist = g['dist_table']
    assert dist[8] == pytest.approx(MEASURED['fdc_slope'], rel=1e-3) and dist[13] == pytest.approx(MEASURED['centroid'], rel=1e-3)
    hi, lo = g['table_{}'.format(years)], g['table_lo_{}'.format(years)]
    assert np.array_equal(np.isnan(table[:, [8, 13]]), np.isnan(hi[:, [8, 13]])), tag
    with np.errstate(invalid='ignore'):
        slope = np.abs((table[:, 8] - hi[:, 8]) - lo[:, 8]) / np.maximum(np.abs(hi[:, 8]), 1.0)
        d = np.abs((table[:, 13] - hi[:, 13]) - lo[:, 13])
        centroid = np.minimum(d, 12.0 - d) * np.where(np.isnan(hi[:, 14]), 1.0, hi[:, 14])
    for name, err, b in (('fdc_slope', slope, max(4.0 * dist[8], 4.0 * EPS)), ('centroid', centroid, max(4.0 * dist[13], 4.0 * 2.0 ** -49))):
        worst = float(np.nanmax(err)) if (~np.isnan(err)).any() else 0.0
        print('{}: {} max error {:.3e}, bound {:.3e}'.format(tag, name, worst, b))
        assert worst <= b, (tag, name, worst, b)


def held(golden, got, ref, years, tag):
    """(table, fdc, regime) of the case rows of ``years`` against the host build's or the restatement's: the same bits in every
    column but two, and those inside their bounds."""
    assert same_bits(got[0][:, BIT_COLUMNS], ref[0][:, BIT_COLUMNS]), tag
    assert same_bits(got[1], ref[1]) and same_bits(got[2], ref[2]), tag
    assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0])), tag
    bounded_columns(golden, got[0], years, tag)


@pytest.fixture(scope='module')
def probe():
    """tests/signatures_probe/libsignatures_probe.so and sort_check (build() makes them; made here when the suite runs without
    it)."""
    path = os.path.join(PROBE_DIR, 'libsignatures_probe.so')
    if not os.path.isfile(path) or not os.path.isfile(os.path.join(PROBE_DIR, 'sort_check')):
        subprocess.run(['make', '-C', PROBE_DIR], check=True, capture_output=True)
    lib = ctypes.CDLL(path)
    lib.sp_signatures.restype = ctypes.c_int
    lib.sp_signatures.argtypes = [ctypes.c_int64] + [ctypes.c_int32] * 5 + [P] * 5
    lib.sp_quantile.restype = None
    lib.sp_quantile.argtypes = [ctypes.c_int32, P, ctypes.c_int64, P, P]
    return lib


def host_signatures(probe, rows, start=0, nyear=None, cal0=cases.CAL0, probs=PROBS, fdc=True, regime=True, fill=-777.0):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    nyear = (rows.shape[1] - start) // 12 if nyear is None else nyear
    probs = np.ascontiguousarray(probs, dtype=np.float64)
    table = np.full((rows.shape[0], snp.NCOL), fill)
    f, m = np.full((rows.shape[0], probs.size), fill), np.full((rows.shape[0], 12), fill)
    rc = probe.sp_signatures(rows.shape[0], rows.shape[1], start, nyear, cal0, probs.size, probs.ctypes.data_as(P) if probs.size else None,
                             rows.ctypes.data_as(P), table.ctypes.data_as(P), f.ctypes.data_as(P) if fdc else None,
                             m.ctypes.data_as(P) if regime else None)
    assert rc == 0
    return table, f, m


@pytest.fixture(scope='module')
def reference():
    """The rows of every year count and their restatement, computed once."""
    return {ny: (cases.rows(ny), snp.signatures(cases.rows(ny), 0, ny, cases.CAL0, PROBS)) for ny in cases.YEARS}


# ------------------------------------------------------------------ the rows and the restatement
def test_the_rows_cover_what_they_should(reference):
    assert cases.YEARS == (1, 2, 5, 21, 22, 43, 86, 341) and len(cases.KINDS) == 15 and snp.COLUMNS[8] == 'fdc_slope'
    k = {name: i for i, name in enumerate(cases.KINDS)}
    for ny, (x, (table, fdc, regime)) in reference.items():
        assert x.shape == (15, 12 * ny)
        assert (table[:, 0] == np.isfinite(x).sum(axis=1)).all()
        assert table[k['all_nan'], 0] == 0 and np.isnan(np.delete(table[k['all_nan']], [0, 1, 15])).all() and np.isnan(fdc[k['all_nan']]).all()
        assert table[k['one_finite'], 0] == 1 and np.isnan(table[k['one_finite'], 3]) and not np.isnan(table[k['one_finite'], 2])
        assert table[k['two_finite'], 0] == 2 and not np.isnan(table[k['two_finite'], 3])
        assert np.isnan(table[k['month_nan'], 9:15]).all() and np.isnan(regime[k['month_nan']]).sum() == 1
        assert table[k['year_nan'], 15] == ny - 1 and table[k['skewed'], 15] == ny
        assert table[k['intermittent'], 1] > 0 and table[k['signed_zeros'], 1] > 0
        assert (np.signbit(x[k['signed_zeros']]) & (x[k['signed_zeros']] == 0)).any() and not np.signbit(fdc[k['signed_zeros']]).any()
        assert np.isnan(table[k['negative'], 8]) or ny == 1
        if ny >= 5:
            assert 0 < table[k['scattered'], 0] < 12 * ny and np.isinf(x[k['scattered']]).any()
            assert not np.isnan(table[k['skewed']]).any() and not np.isnan(table[k['seasonal']]).any()
            assert table[k['seasonal'], 12] > table[k['constant'], 12] and table[k['seasonal'], 14] > 0.3


def test_duration_curve_and_median_are_np_quantile_bit_for_bit(reference):
    for ny, (x, (table, fdc, regime)) in reference.items():
        for i, row in enumerate(x):
            v = (row + 0.0)[np.isfinite(row)]
            if v.size:
                assert same_bits(fdc[i], np.quantile(v, PROBS, method='linear')), (ny, cases.KINDS[i])
                assert same_bits(table[i, 5], np.quantile(v, 0.5, method='linear')), (ny, cases.KINDS[i])
                assert same_bits(table[i, 5], np.median(v)) or v.size % 2 == 0       # (an odd count: the middle value itself)


def test_moments_against_numpy(reference):
    """mean, std and the annual columns within a few ulp x n of np.mean and np.std(ddof=1), which sum pairwise: the bound is
    4 (n + 16) 2^-53 of the row's largest magnitude (12 of them for an annual total), as at `tolerances`."""
    for ny, (x, (table, fdc, regime)) in reference.items():
        for i, row in enumerate(x):
            v = row[np.isfinite(row)]
            if v.size < 2:
                continue
            tol = 4.0 * (v.size + 16) * 2.0 ** -53 * np.abs(v).max()
            assert abs(table[i, 2] - np.mean(v)) <= tol and abs(table[i, 3] - np.std(v, ddof=1)) <= 2.0 * tol, (ny, cases.KINDS[i])
            years = row.reshape(ny, 12)
            A = years[np.isfinite(years).all(axis=1)].sum(axis=1)
            if A.size >= 2:
                assert abs(table[i, 16] - np.mean(A)) <= 12.0 * tol, (ny, cases.KINDS[i])
                cv = np.std(A, ddof=1) / np.mean(A)
                assert abs(table[i, 17] - cv) <= 24.0 * tol / abs(np.mean(A)) * (1.0 + abs(cv)), (ny, cases.KINDS[i])


def tolerances(x, g):
    """The bound on |value - 40-digit value| per column of one row: 8 E scale, E = (12 nyear + 16) 2^-53 the rounding of a sum of
    that many terms, X the row's largest magnitude.  A sum of n terms of magnitude <= X divided by n errs by E X: mean, the
    calendar means, the order statistics (an interpolation of two elements: a few ulp of X); 12 of them by 12 E X:
    regime_total, annual_mean.  A deviation x - mean errs by d = E X, a sum of squares s of n of them by 2 d sum|dev|, its
    root by 1.5 d (Cauchy-Schwarz), or by d itself where s = 0: std.  A quotient N / D errs by (dN + |N / D| dD) / |D|: cv (X /
    |mean|), lag1 (dN = 4 E n X^2 over s), flashiness (2 n X over the sum), seasonality and concentration (24 X / |R|),
    annual_cv (24 X / |annual_mean|), each times (1 + |quotient|)."""
    keep = np.isfinite(x)
    X = float(np.abs(x[keep]).max()) if keep.any() else 0.0
    n = float(keep.sum())
    E = (x.size + 16) * 2.0 ** -53
    with np.errstate(all='ignore'):
        sxx = g[3] ** 2 * (n - 1.0)
        scale = np.array([0.0, 0.0, X, 1.5 * X, X / abs(g[2]) * (1 + abs(g[4])), X, 4 * n * X * X / sxx * (1 + abs(g[6])),
                          2 * n * X / abs(g[2] * n) * (1 + abs(g[7])), np.nan, 12 * X, 0.0, 0.0, 24 * X / abs(g[9]) * (1 + abs(g[12])),
                          np.nan, 24 * X / abs(g[9]) * (1 + abs(g[14])), 0.0, 12 * X, 24 * X / abs(g[16]) * (1 + abs(g[17]))])
    return 8.0 * E * scale, 8.0 * E * X


@pytest.mark.parametrize('years', cases.YEARS)
def test_restatement_and_host_build_against_40_digits(probe, reference, golden, years):
    g = golden('signatures')
    x, ref = reference[years]
    hi, lo, undef = g['table_{}'.format(years)], g['table_lo_{}'.format(years)], g['undef_{}'.format(years)]
    for name, (table, fdc, regime) in (('restatement', ref), ('host build', host_signatures(probe, x))):
        tag = '{} {}'.format(name, years)
        assert np.array_equal(np.isnan(table) & ~undef, np.isnan(hi) & ~undef), tag
        for i, row in enumerate(x):
            tol, tol_x = tolerances(row, hi[i])
            err = np.abs((table[i] - hi[i]) - lo[i])
            for c in BIT_COLUMNS:
                if not np.isnan(hi[i, c]) and not undef[i, c]:
                    assert err[c] <= tol[c], (tag, cases.KINDS[i], snp.COLUMNS[c], err[c], tol[c])
            for got, what in ((fdc, 'fdc'), (regime, 'regime')):
                e = np.abs((got[i] - g['{}_{}'.format(what, years)][i]) - g['{}_lo_{}'.format(what, years)][i])
                assert np.array_equal(np.isnan(got[i]), np.isnan(g['{}_{}'.format(what, years)][i])), (tag, cases.KINDS[i], what)
                assert not (e > tol_x).any(), (tag, cases.KINDS[i], what, np.nanmax(e), tol_x)
        bounded_columns(golden, table, years, tag)


# ------------------------------------------------------------------ the host build of the header
@pytest.mark.parametrize('years', cases.YEARS)
def test_host_build_of_the_header_against_the_restatement(probe, reference, golden, years):
    x, ref = reference[years]
    held(golden, host_signatures(probe, x), ref, years, 'host build {}'.format(years))


def test_window_stride_calendar_and_probabilities(probe):
    wide = cases.rows(22)
    wide = np.concatenate([wide[:, -7:], wide, wide[:, :10]], axis=1)
    sixteen = np.linspace(0.03, 0.97, 16)
    for start, nyear, cal0, probs in ((0, 22, 0, PROBS), (7, 22, 3, sixteen), (17, 21, 11, np.array([])), (9, 12, 6, np.array([0.5]))):
        got = host_signatures(probe, wide, start, nyear, cal0, probs)
        ref = snp.signatures(wide, start, nyear, cal0, probs)
        assert got[1].shape == (15, probs.size)
        assert same_bits(got[0][:, BIT_COLUMNS], ref[0][:, BIT_COLUMNS]) and same_bits(got[1], ref[1]) and same_bits(got[2], ref[2])
        assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0]))
    # the calendar: a window that starts cal0 months into the year has the regime rolled by cal0
    x = cases.rows(5)[:2]
    a, b = host_signatures(probe, x, cal0=0), host_signatures(probe, x, cal0=4)
    assert same_bits(np.roll(a[2], 4, axis=1), b[2]) and same_bits(a[0][:, :9], b[0][:, :9]) and same_bits(a[0][:, 15:], b[0][:, 15:])
    assert ((b[0][:, 10] - a[0][:, 10]) % 12 == 4).all()
    # NULL outputs are left alone
    full = host_signatures(probe, wide, 7, 22)
    for fdc, regime in ((False, True), (True, False), (False, False)):
        got = host_signatures(probe, wide, 7, 22, fdc=fdc, regime=regime)
        assert got[0].tobytes() == full[0].tobytes()
        assert got[1].tobytes() == full[1].tobytes() if fdc else (got[1] == -777.0).all()
        assert got[2].tobytes() == full[2].tobytes() if regime else (got[2] == -777.0).all()


def test_probe_refuses_what_the_entry_refuses(probe):
    x, t = np.ones((2, 130)), np.full((2, snp.NCOL), -777.0)
    f, m = np.full((2, 16), -777.0), np.full((2, 12), -777.0)
    p = np.array([0.5, 0.9])

    def rc(stride=130, col0=0, nyear=10, cal0=0, nP=2, prob=p, rows=x, table=t):
        return probe.sp_signatures(2, stride, col0, nyear, cal0, nP, None if prob is None else prob.ctypes.data_as(P),
                                   None if rows is None else rows.ctypes.data_as(P), None if table is None else table.ctypes.data_as(P),
                                   f.ctypes.data_as(P), m.ctypes.data_as(P))
    for bad in (dict(rows=None), dict(table=None), dict(prob=None), dict(col0=-1), dict(col0=11), dict(nyear=0), dict(nyear=342, stride=5000),
                dict(cal0=-1), dict(cal0=12), dict(nP=-1), dict(nP=17), dict(prob=np.array([0.5, 1.0])), dict(prob=np.array([0.0, 0.5])),
                dict(prob=np.array([np.nan, 0.5]))):
        assert rc(**bad) == 1, bad
    assert (t == -777.0).all() and (f == -777.0).all() and (m == -777.0).all()
    assert rc() == 0 and rc(nP=0, prob=None) == 0 and (t[:, 0] == 120).all()


def test_sort_and_order_statistics_under_sanitizers(probe):
    """xh_sig_load, xh_sig_sort and xh_sig_quantile in a stand-alone program of their own (tests/signatures_probe/sort_check.cpp,
    -fsanitize=address,undefined), started as a child process: series of 1 .. 4096 elements with ties, signed zeros, NaN and
    infinite elements, ascending and descending ones, teams of 1, 3 and 256 lanes, in buffers of exactly the sizes the kernel
    gives a workgroup, against std::sort."""
    out = subprocess.run([os.path.join(PROBE_DIR, 'sort_check'), '300', '20263'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and '300 cases, 0 failed' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_order_statistic_is_np_quantile_over_many_lengths(probe):
    rng = np.random.default_rng(11)
    p = np.ascontiguousarray(np.concatenate([(100.0 - np.arange(1, 100)) / 100.0, [0.34, 0.67]]))
    for n in list(range(1, 40)) + [255, 256, 257, 600, 1023, 4092, 4096]:
        a = np.sort(np.round(rng.gamma(0.5, 10.0, n), int(rng.integers(0, 7))))
        q = np.full(p.size, -777.0)
        probe.sp_quantile(n, a.ctypes.data_as(P), p.size, p.ctypes.data_as(P), q.ctypes.data_as(P))
        assert same_bits(q, np.quantile(a, p, method='linear')), n


# ------------------------------------------------------------------ the section
NM = 144


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('signatures_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = synth.make_forcing(w, NM, seed=50)
    plain = synth.write_example(root, w, f, 1971, 1982, runoff_spinup=25, routing_spinup=6)
    ini = synth.write_example(root, w, f, 1971, 1982, runoff_spinup=25, routing_spinup=6, project='with_signatures')
    synth.with_signatures(ini, signature_vars=('q', 'avgchflow'))
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
    assert '[Signatures]' in msg and all(k in msg for k in keys), msg
    return msg


VARS_LINE = r'signature_vars = q, avgchflow'


def test_section_and_its_defaults(tree, tmp_path):
    root, w, f, plain, ini = tree
    from xanthos_amd import signatures
    c = ConfigReader(ini)
    assert c.CalculateSignatures == 1
    assert c.signatures == {'vars': ['q', 'avgchflow'], 'exceedance': [1.0, 5.0, 10.0, 20.0, 50.0, 80.0, 90.0, 95.0, 99.0],
                            'start_year': 1971, 'end_year': 1982, 'year_start_month': 1}
    c = ConfigReader(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = PET, aet, soilmoisture, precip\nexceedance = 0.5, 95\n'
                                            'year_start_month = 10\nstart_year = 1972')))
    assert c.signatures['vars'] == ['pet', 'aet', 'soilmoisture', 'precip'] and c.signatures['exceedance'] == [0.5, 95.0]
    # the year that starts in October 1981 is the last that ends inside 1982
    assert (c.signatures['start_year'], c.signatures['end_year'], c.signatures['year_start_month']) == (1972, 1981, 10)
    assert os.path.basename(signatures.output_stem(c, 'q')) == 'signatures_q_with_signatures'
    assert os.path.basename(signatures.output_stem(c, 'q', 'fdc')) == 'signatures_q_fdc_with_signatures'
    assert signatures.COLUMNS == snp.COLUMNS and signatures.EXCEEDANCE == snp.EXCEEDANCE == cases.EXCEEDANCE and len(signatures.COLUMNS) == 18
    assert same_bits(signatures.probabilities(), PROBS) and signatures.exceedance_name(95.0) == 'Q95' and signatures.exceedance_name(0.5) == 'Q0.5'


def test_an_ini_without_the_flag_parses_as_before(tree):
    root, w, f, plain, ini = tree
    base = vars(ConfigReader(plain))
    assert base['CalculateSignatures'] == 0 and base['signatures'] is None and 'Signatures' not in open(plain).read()
    with_flag = vars(ConfigReader(ini))
    differ = sorted(k for k in base if k not in ('CalculateSignatures', 'signatures') and repr(base[k]) != repr(with_flag[k]))
    assert all('with_signatures' in repr(with_flag[k]) for k in differ), differ       # only the project's name and its folders


def test_with_signatures_writes_the_section(tree, tmp_path):
    root, w, f, plain, ini = tree
    path = str(tmp_path / 'enabled.ini')
    open(path, 'w').write(open(plain).read())
    assert synth.with_signatures(path, signature_vars=('q',), exceedance=(5, 95), year_start_month=4, start_year=1973) == path
    text = open(path).read()
    assert 'CalculateSignatures = 1' in text.split('[PET]')[0] and text.rstrip().endswith('start_year = 1973')
    assert '[Signatures]\nsignature_vars = q\nexceedance = 5, 95\nyear_start_month = 4' in text
    c = ConfigReader(path)
    assert c.signatures['exceedance'] == [5.0, 95.0] and (c.signatures['start_year'], c.signatures['end_year']) == (1973, 1981)


def test_refusals_name_their_key(tree, tmp_path):
    root, w, f, plain, ini = tree
    refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q, chstorage')), 'signature_vars', 'chstorage')
    refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q, q')), 'signature_vars')
    refused(edited(ini, tmp_path, (VARS_LINE + r'\n', '')), 'signature_vars')
    refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q\nmin_years = 10')), 'min_years', 'not a key')
    # avgchflow without routing
    msg = refused(edited(ini, tmp_path, (r'(?s)\[Routing\].*?\n\[Signatures\]', '[Signatures]')), 'signature_vars', 'avgchflow')
    assert 'routing_module' in msg
    # precip (and q) without a runoff module
    no_runoff = ((r'(?s)\[Runoff\].*?\n\[Routing\]', '[Routing]'), (r'(?s)\[Routing\].*?\n\[Signatures\]', '[Signatures]'))
    for var in ('precip', 'q', 'aet', 'soilmoisture'):
        msg = refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = ' + var), *no_runoff), 'signature_vars', var)
        assert 'runoff_module' in msg
    # pet without the module that makes it: PET from a file
    pet_file = os.path.join(root, 'pet.npy')
    np.save(pet_file, np.ones((w.ncell, NM)))
    msg = refused(edited(ini, tmp_path, (r'(?s)\[PET\].*?\n\[Runoff\]', '[PET]\npet_module = none\npet_file = {}\n\n[Runoff]'.format(
        pet_file)), (VARS_LINE, 'signature_vars = pet')), 'signature_vars', 'pet')
    assert 'pet_module' in msg
    # the window
    refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q\nstart_year = 1970')), 'start_year', '1970')
    refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q\nend_year = 1983')), 'end_year', '1983')
    refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q\nstart_year = soon')), 'start_year', 'soon')
    refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q\nstart_year = 1975\nend_year = 1974')), 'end_year', '1974', '1975')
    # an incomplete last year
    msg = refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q\nyear_start_month = 10\nend_year = 1982')), 'end_year', '1982', 'month 10')
    assert '1981' in msg
    for bad in ('0', '13', 'october'):
        refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q\nyear_start_month = ' + bad)), 'year_start_month', bad)
    for bad in ('0', '100', '-5, 10', '10, 10', ', '.join(str(p) for p in range(1, 18)), 'often', 'nan', '1e-20'):
        refused(edited(ini, tmp_path, (VARS_LINE, 'signature_vars = q\nexceedance = ' + bad)), 'exceedance')
    refused(edited(ini, tmp_path, (r'OutputInYear = 0', 'OutputInYear = 1')), 'OutputInYear')
    # the flag and the section
    with pytest.raises(ValidationException, match='CalculateSignatures'):
        ConfigReader(edited(ini, tmp_path, (r'CalculateSignatures = 1', 'CalculateSignatures = yes')))
    with pytest.raises(ValidationException, match=r'CalculateSignatures = 1 but the config file has no \[Signatures\] section'):
        ConfigReader(edited(ini, tmp_path, (r'(?s)\n\[Signatures\].*$', '\n')))


def test_a_window_beyond_4096_months_is_refused(tree):
    root, w, f, plain, ini = tree
    c = ConfigReader(ini)
    c.StartYear, c.EndYear = 1700, 2041
    with pytest.raises(ValidationException) as exc:
        c.configure_signatures({'signature_vars': 'q'})
    assert '[Signatures] end_year' in str(exc.value) and '4104 months' in str(exc.value) and '4096' in str(exc.value)
    c.configure_signatures({'signature_vars': 'q', 'year_start_month': '10'})          # 341 years
    assert c.signatures['end_year'] == 2040


def test_calibration_ensembles_and_sharded_precipitation_are_refused(tree, tmp_path):
    root, w, f, plain, ini = tree
    c = ConfigReader(ini)
    c.calibrate = 1
    with pytest.raises(ValidationException, match=r'\[Signatures\] and Calibrate = 1'):
        c.configure_signatures({'signature_vars': 'q'})
    c.calibrate = 0
    c.ensemble = {'members': 'members.csv'}
    with pytest.raises(ValidationException, match=r'\[Signatures\] and an \[Ensemble\] section'):
        c.configure_signatures({'signature_vars': 'q'})
    with_ens = edited(ini, tmp_path, (r'(?s)$', '\n[Ensemble]\nmembers = members.csv\n'), name='ens.ini')
    try:
        ConfigReader(with_ens)
    except ValidationException as exc:          # whichever section speaks first, the run does not start
        assert '[Signatures]' in str(exc) or '[Ensemble]' in str(exc)
    else:
        raise AssertionError('an ini with [Signatures] and [Ensemble] was accepted')
    from xanthos_amd import ensemble
    with pytest.raises(ValidationException) as exc:
        ensemble.validate(ConfigReader(ini), [('a', {})])
    assert 'CalculateSignatures' in str(exc.value) and '[Ensemble]' in str(exc.value)
    # precip in a sharded run: every rank's pipeline holds its own rows only
    from types import SimpleNamespace
    from xanthos_amd.components import Components
    comp = Components.__new__(Components)
    comp.s = SimpleNamespace(ncell=w.ncell, nmonths=NM)
    comp.pipe = SimpleNamespace(forcing={'precip': SimpleNamespace(shape=(w.ncell // 2, NM))})
    with pytest.raises(ValidationException) as exc:
        comp._precipitation('precip', 'Signatures')
    assert '[Signatures] signature_vars = precip' in str(exc.value)


# ------------------------------------------------------------------ the C-ABI entry
def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    assert re.search(r'\bint xh_signatures\(xh_ctx \*ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t cal0, '
                     r'int32_t nP,\s+const double \*h_prob, const double \*d_x, double \*d_table, double \*d_fdc, double \*d_regime\);', header)
    assert re.search(r'#define XH_SIG_NCOL 18\b', header) and re.search(r'#define XH_SIG_MAX_P 16\b', header)
    assert 'xh_signatures replaces NO function of the reference' in header
    assert len(_hip.SIGNATURES['xh_signatures'][1]) == 12
    assert hasattr(_hip.lib(), 'xh_signatures') and _hip.lib().xh_abi_version() == _hip.ABI_VERSION == 7
    assert hasattr(_hip.Context, 'signatures')
    dev = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'xh_signatures_dev.h')).read()
    assert re.search(r'#define XH_SIG_NCOL 18\b', dev) and '__host__ __device__' in dev
    assert re.search(r'#define XH_SIG_MONTHS_PER_RADIAN {!r}\b'.format(snp.MONTHS_PER_RADIAN), dev)
    import mpmath as mp
    mp.mp.dps = 50
    for name, table, fn in (('c', snp.COS, mp.cos), ('s', snp.SIN, mp.sin)):
        block = re.search(r'const double {}\[12\] = \{{(.*?)\}};'.format(name), dev, re.S).group(1)   # the header's literals are the
        lits = [float(v) for v in block.replace('\n', ' ').split(',')]                              # restatement's, correctly rounded
        assert lits == list(table) == [float(fn(mp.pi * (2 * m + 1) / 12)) for m in range(12)]
    assert snp.MONTHS_PER_RADIAN == float(6 / mp.pi)
    make = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'Makefile')).read()
    assert 'xh_signatures.hip' in make and 'xh_signatures.o: xh_signatures.hip $(HDRS) xh_signatures_dev.h' in make
