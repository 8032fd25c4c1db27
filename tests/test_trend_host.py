"""Mann-Kendall test and Theil-Sen slope per row, everything a machine without a GPU can check: the numpy
restatement (tests/trend_np.py) against scipy.stats.theilslopes bit for bit, the host build of csrc/xh_trend_dev.h
(tests/trend_probe) against the restatement, z and p against 40-digit values, the radix select against std::sort under the
sanitizers, the [Trend] section's refusals and the C-ABI bookkeeping.

The bound on p.  p = erfc(|z| / sqrt 2) magnifies the rounding of z and of the product by erfc's condition number, about
z^2: every float64 evaluation shares that error.  tests/golden/make_golden_trend.py measures it for scipy's erfc against the
40-digit values on these very rows: 7.099e-14 relative (319.7 ulp, at the monotone annual row of 257 years, z = 23.9).  The
bound is 4 x that = 2.84e-13 (the margin because the device's erfc is another implementation), and not below 4 ulp."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import trend_cases as cases
import trend_np
from xanthos_amd import ConfigReader, ValidationException, _hip, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PROBE_DIR = os.path.join(ROOT, 'tests', 'trend_probe')
P = ctypes.c_void_p
EPS = float(np.finfo(np.float64).eps)


def p_bound(golden):
    measured = float(golden('trend')['scipy_p_relerr'])
    assert measured == pytest.approx(7.099e-14, rel=1e-3)          # the figure of the docstring
    return max(4.0 * measured, 4.0 * EPS)


@pytest.fixture(scope='module')
def probe():
    """tests/trend_probe/libtrend_probe.so and select_check (build() makes them; made here when the suite runs without it)."""
    path = os.path.join(PROBE_DIR, 'libtrend_probe.so')
    if not os.path.isfile(path) or not os.path.isfile(os.path.join(PROBE_DIR, 'select_check')):
        subprocess.run(['make', '-C', PROBE_DIR], check=True, capture_output=True)
    lib = ctypes.CDLL(path)
    lib.tp_trend.restype = ctypes.c_int
    lib.tp_trend.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, P, P]
    return lib


def host_trend(probe, rows, nseason, z_conf=cases.Z95, start=0, ncol=None):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ncol = rows.shape[1] - start if ncol is None else ncol
    out = np.full((rows.shape[0], 10), -777.0)
    rc = probe.tp_trend(rows.shape[0], rows.shape[1], start, ncol, nseason, z_conf, rows.ctypes.data_as(P), out.ctypes.data_as(P))
    assert rc == 0
    return out


@pytest.fixture(scope='module')
def reference():
    """trend_np of the host rows of every shape, computed once."""
    return {(ns, ny): trend_np.trend_rows(cases.make_rows(ns, ny, cases.HOST_ROWS), ns, cases.Z95) for ns, ny in cases.SHAPES}


# ------------------------------------------------------------------ (a) the restatement against scipy
def test_restatement_is_scipy_theilslopes_bit_for_bit():
    from scipy import stats
    checked = 0
    for years in cases.YEARS:
        rows = cases.make_rows(1, years, cases.HOST_ROWS)
        for conf in (0.95, 0.8):
            z_conf = float(stats.norm.ppf((1.0 - conf) / 2.0))
            for r, x in enumerate(rows):
                if not np.isfinite(x).all():
                    continue
                got = trend_np.trend_row(x, 1, z_conf)
                want = stats.theilslopes(x, np.arange(x.size), conf)
                for a, b in zip(got[[5, 6, 7, 8]], want):
                    # (scipy keeps a slope of -0.0, the definition counts it as +0.0: bits of everything else)
                    assert (a == 0.0 and b == 0.0) or np.float64(a).tobytes() == np.float64(b).tobytes(), (years, r, conf, got, want)
                checked += 1
    kinds = {cases.KINDS[r % len(cases.KINDS)] for r in range(cases.HOST_ROWS)}
    assert {'tied', 'constant', 'signed_zeros'} <= kinds and checked >= 6 * 2 * 14


# ------------------------------------------------------------------ (b) the host build of the header
@pytest.mark.parametrize('nseason,years', cases.SHAPES)
def test_host_build_of_the_header_against_the_restatement(probe, reference, nseason, years):
    rows = cases.make_rows(nseason, years, cases.HOST_ROWS)
    got, ref = host_trend(probe, rows, nseason), reference[(nseason, years)]
    assert cases.same_but_p(got, ref), np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    assert got[:, 3].tobytes() == ref[:, 3].tobytes()                        # z bit for bit
    few = [r for r in range(cases.HOST_ROWS) if cases.KINDS[r % len(cases.KINDS)] == 'few']
    assert (got[few, 0] < 4).all() and np.isnan(got[few, 1:9]).all() and not np.isnan(got[few][:, [0, 9]]).any()
    const = [r for r in range(cases.HOST_ROWS) if cases.KINDS[r % len(cases.KINDS)] == 'constant']
    assert (got[const][:, [1, 2, 3, 5, 7, 8]] == 0.0).all() and (got[const, 4] == 1.0).all()


def test_window_inside_a_longer_row(probe):
    rng = np.random.default_rng(5)
    wide = rng.normal(size=(7, 12 * 30 + 17))
    wide[2, 40:90] = np.nan
    for nseason, start, ncol in ((12, 5, 12 * 22), (12, 24, 12 * 28), (1, 3, 64), (4, 17, 4 * 65)):
        got = host_trend(probe, wide, nseason, start=start, ncol=ncol)
        ref = trend_np.trend_rows(wide, nseason, cases.Z95, start, ncol)
        assert cases.same_but_p(got, ref) and got[:, 3].tobytes() == ref[:, 3].tobytes()
    other = host_trend(probe, wide, 12, z_conf=-0.8416212335729143, start=5, ncol=12 * 22)
    ref = trend_np.trend_rows(wide, 12, -0.8416212335729143, 5, 12 * 22)
    assert cases.same_but_p(other, ref) and not np.array_equal(other[:, 7:9], got[:, 7:9])


def test_probe_refuses_what_the_entry_refuses(probe):
    x = np.zeros((2, 24))
    out = np.full((2, 10), -777.0)
    for stride, col0, ncol, ns, z in ((24, -1, 12, 1, -1.96), (24, 13, 12, 12, -1.96), (24, 0, 20, 12, -1.96), (24, 0, 0, 1, -1.96),
                                      (24, 0, 24, 0, -1.96), (24, 0, 24, 13, -1.96), (24, 0, 24, 12, 1.96), (24, 0, 24, 12, 0.0),
                                      (24, 0, 24, 12, float('nan')), (24, 0, 24, 12, float('-inf'))):
        assert probe.tp_trend(2, stride, col0, ncol, ns, z, x.ctypes.data_as(P), out.ctypes.data_as(P)) == 1
    assert (out == -777.0).all()


# ------------------------------------------------------------------ (c) z and p against 40 digits
@pytest.mark.parametrize('nseason,years', cases.SHAPES)
def test_z_and_p_against_40_digits(probe, reference, golden, nseason, years):
    g = golden('trend')
    gz, gp = g['z_{}_{}'.format(nseason, years)], g['p_{}_{}'.format(nseason, years)]
    bound = p_bound(golden)
    ref = reference[(nseason, years)]
    got = host_trend(probe, cases.make_rows(nseason, years, cases.HOST_ROWS), nseason)
    tiny = np.flatnonzero(gp < cases.TINY)
    monotone = [r for r in range(cases.HOST_ROWS) if cases.KINDS[r % len(cases.KINDS)] in ('increasing', 'decreasing')]
    # p lies below the smallest normal double for the strictly monotone seasonal rows of 64 and more years, and for no others
    # (64 years: S = 24192, var_s = 357504, z = 40.46, p = 1e-357, which no double holds: the weaker demand starts there, one
    # year before the 65 the feature's description names)
    assert list(tiny) == (monotone if nseason == 12 and years >= 64 else [])
    for table in (ref, got):
        assert np.array_equal(np.isnan(table[:, 3]), np.isnan(gz))
        ok = ~np.isnan(gz)
        err_z = np.abs(table[ok, 3] - gz[ok])
        print('z: max error {:.2f} ulp'.format(float((err_z / np.maximum(np.spacing(np.abs(gz[ok])), 5e-324)).max()) if ok.any() else 0.0))
        assert (err_z <= 2.0 * np.spacing(np.abs(gz[ok]))).all()          # a square root and a division, the golden rounded once
        rest = ok & (gp >= cases.TINY)
        if rest.any():
            print('p: max relative error {:.3e}, bound {:.3e}'.format(
                float((np.abs(table[rest, 4] - gp[rest]) / gp[rest]).max()), bound))
        assert cases.p_within(table[:, 4], gp, bound)


# ------------------------------------------------------------------ (d) the selection under the sanitizers
def test_radix_select_against_std_sort_under_sanitizers(probe):
    """xh_tr_select, XhTrSlopes and xh_trend_row in a stand-alone program of their own (tests/trend_probe/select_check.cpp,
    -fsanitize=address,undefined), started as a child process: virtual arrays with ties, signed zeros, N = 1, 2, 255, 256,
    257 and the extreme ranks; the slope array against two plain loops, in buffers of exactly the sizes the kernel has."""
    out = subprocess.run([os.path.join(PROBE_DIR, 'select_check'), '600', '20261'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and '600 cases of each kind, 0 failed' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ------------------------------------------------------------------ (e) the section
NM = 72


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('trend_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = synth.make_forcing(w, NM, seed=50)
    plain = synth.write_example(root, w, f, 1971, 1976, runoff_spinup=25, routing_spinup=6)
    ini = synth.write_example(root, w, f, 1971, 1976, runoff_spinup=25, routing_spinup=6, project='with_trend')
    synth.enable_trend(ini, trend_vars=('q', 'avgchflow'), series=('annual', 'seasonal'))
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
    assert '[Trend]' in msg and all(k in msg for k in keys), msg
    return msg


def test_section_and_its_defaults(tree, tmp_path):
    root, w, f, plain, ini = tree
    from xanthos_amd import trend
    c = ConfigReader(ini)
    assert c.CalculateTrend == 1
    assert c.trend == {'vars': ['q', 'avgchflow'], 'series': ['annual', 'seasonal'], 'annual': trend.ANNUAL_DEFAULT,
                       'start_year': 1971, 'end_year': 1976, 'confidence': 0.95}
    assert trend.ANNUAL_DEFAULT == {'q': 'sum', 'pet': 'sum', 'aet': 'sum', 'precip': 'sum', 'soilmoisture': 'mean', 'avgchflow': 'mean'}
    c = ConfigReader(edited(ini, tmp_path, (r'trend_vars = q, avgchflow', 'trend_vars = PET, aet, soilmoisture, precip'),
                            (r'series = annual, seasonal', 'series = Seasonal\nannual = mean\nstart_year = 1972\nend_year = 1975\n'
                                                           'confidence = 0.9')))
    assert c.trend['vars'] == ['pet', 'aet', 'soilmoisture', 'precip'] and c.trend['series'] == ['seasonal']
    assert set(c.trend['annual'].values()) == {'mean'} and (c.trend['start_year'], c.trend['end_year']) == (1972, 1975)
    assert c.trend['confidence'] == 0.9
    assert os.path.basename(trend.output_stem(c, 'q', 'annual')) == 'trend_q_annual_with_trend'
    assert trend.COLUMNS == trend_np.COLUMNS and len(trend.COLUMNS) == 10
    from statistics import NormalDist
    assert trend.z_of(0.95) == NormalDist().inv_cdf((1 - 0.95) / 2) and abs(trend.z_of(0.95) - cases.Z95) < 1e-14
    base = vars(ConfigReader(plain))
    assert base['CalculateTrend'] == 0 and base['trend'] is None and 'Trend' not in open(plain).read()


def test_refusals_name_their_key(tree, tmp_path):
    root, w, f, plain, ini = tree
    refused(edited(ini, tmp_path, (r'trend_vars = q, avgchflow', 'trend_vars = q, chstorage')), 'trend_vars', 'chstorage')
    refused(edited(ini, tmp_path, (r'trend_vars = q, avgchflow\n', '')), 'trend_vars')
    refused(edited(ini, tmp_path, (r'series = annual, seasonal', 'series = annual, monthly')), 'series', 'monthly')
    refused(edited(ini, tmp_path, (r'series = annual, seasonal\n', '')), 'series')
    refused(edited(ini, tmp_path, (r'series = annual, seasonal', 'series = annual\nannual = median')), 'annual', 'median')
    # avgchflow without routing
    msg = refused(edited(ini, tmp_path, (r'(?s)\[Routing\].*?\n\[Trend\]', '[Trend]')), 'trend_vars', 'avgchflow')
    assert 'routing_module' in msg
    # precip (and q) without a runoff module
    no_runoff = ((r'(?s)\[Runoff\].*?\n\[Routing\]', '[Routing]'), (r'(?s)\[Routing\].*?\n\[Trend\]', '[Trend]'))
    for var in ('precip', 'q', 'aet', 'soilmoisture'):
        msg = refused(edited(ini, tmp_path, (r'trend_vars = q, avgchflow', 'trend_vars = ' + var), *no_runoff), 'trend_vars', var)
        assert 'runoff_module' in msg
    # pet without the module that makes it: PET from a file
    pet_file = os.path.join(root, 'pet.npy')
    np.save(pet_file, np.ones((w.ncell, NM)))
    msg = refused(edited(ini, tmp_path, (r'(?s)\[PET\].*?\n\[Runoff\]', '[PET]\npet_module = none\npet_file = {}\n\n[Runoff]'.format(
        pet_file)), (r'trend_vars = q, avgchflow', 'trend_vars = pet')), 'trend_vars', 'pet')
    assert 'pet_module' in msg
    # the window
    refused(edited(ini, tmp_path, (r'series = annual, seasonal', 'series = annual\nstart_year = 1970')), 'start_year', '1970')
    refused(edited(ini, tmp_path, (r'series = annual, seasonal', 'series = annual\nend_year = 1977')), 'end_year', '1977')
    refused(edited(ini, tmp_path, (r'series = annual, seasonal', 'series = annual\nstart_year = 1974')), 'end_year', '4 years')
    refused(edited(ini, tmp_path, (r'series = annual, seasonal', 'series = annual\nend_year = 1973')), 'end_year', '4 years')
    refused(edited(ini, tmp_path, (r'series = annual, seasonal', 'series = annual\nstart_year = soon')), 'start_year', 'soon')
    for bad in ('0.5', '1', '95', 'high'):
        refused(edited(ini, tmp_path, (r'series = annual, seasonal', 'series = annual\nconfidence = ' + bad)), 'confidence', bad)
    # the flag and the section
    with pytest.raises(ValidationException, match='CalculateTrend'):
        ConfigReader(edited(ini, tmp_path, (r'CalculateTrend = 1', 'CalculateTrend = yes')))
    with pytest.raises(ValidationException, match=r'CalculateTrend = 1 but the config file has no \[Trend\] section'):
        ConfigReader(edited(ini, tmp_path, (r'(?s)\n\[Trend\].*$', '\n')))


def test_a_seasonal_window_beyond_4096_months_is_refused(tree):
    """342 years of months do not fit one row of xh_trend: refused by key, while the annual series of the same window passes.
    (No run of that length is staged: the section's check runs on a reader whose years are set.)"""
    root, w, f, plain, ini = tree
    c = ConfigReader(ini)
    c.StartYear, c.EndYear = 1700, 2041
    with pytest.raises(ValidationException) as exc:
        c.configure_trend({'trend_vars': 'q', 'series': ['annual', 'seasonal']})
    assert '[Trend] series' in str(exc.value) and '4104 months' in str(exc.value) and '4096' in str(exc.value)
    c.configure_trend({'trend_vars': 'q', 'series': 'annual'})
    assert c.trend['series'] == ['annual'] and c.trend['end_year'] == 2041
    c.EndYear = 2040
    c.configure_trend({'trend_vars': 'q', 'series': 'seasonal'})


def test_calibration_and_ensembles_are_refused(tree, tmp_path):
    root, w, f, plain, ini = tree
    c = ConfigReader(ini)
    c.calibrate = 1
    with pytest.raises(ValidationException, match=r'\[Trend\] and Calibrate = 1'):
        c.configure_trend({'trend_vars': 'q', 'series': 'annual'})
    c.calibrate = 0
    c.ensemble = {'members': 'members.csv'}
    with pytest.raises(ValidationException, match=r'\[Trend\] and an \[Ensemble\] section'):
        c.configure_trend({'trend_vars': 'q', 'series': 'annual'})
    # an ini with both sections
    with_ens = edited(ini, tmp_path, (r'(?s)$', '\n[Ensemble]\nmembers = members.csv\n'), name='ens.ini')
    try:
        ConfigReader(with_ens)
    except ValidationException as exc:          # whichever section speaks first, the run does not start
        assert '[Trend]' in str(exc) or '[Ensemble]' in str(exc)
    else:
        raise AssertionError('an ini with [Trend] and [Ensemble] was accepted')
    # run_ensemble(members=...) on an ini without the section
    from xanthos_amd import ensemble
    with pytest.raises(ValidationException) as exc:
        ensemble.validate(ConfigReader(ini), [('a', {})])
    assert 'CalculateTrend' in str(exc.value) and '[Ensemble]' in str(exc.value)


# ------------------------------------------------------------------ the C-ABI entry
def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    assert re.search(r'\bint xh_trend\(xh_ctx \*ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t ncol, int32_t nseason, '
                     r'double z_conf,\s+const double \*d_x, double \*d_out\);', header)
    assert re.search(r'#define XH_TREND_NCOL 10\b', header) and 'xh_trend replaces NO function of the reference' in header
    assert len(_hip.SIGNATURES['xh_trend'][1]) == 9
    assert hasattr(_hip.lib(), 'xh_trend') and _hip.lib().xh_abi_version() == _hip.ABI_VERSION == 7
    assert hasattr(_hip.Context, 'trend')
    dev = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'xh_trend_dev.h')).read()
    assert re.search(r'#define XH_TREND_NCOL 10\b', dev) and '__host__ __device__' in dev
