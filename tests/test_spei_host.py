"""CPU checks of SPI / SPEI and the log-logistic distribution: the numpy restatement (spei_np) against the 40-digit
golden; the fit and the distribution function of csrc/xh_sindex_dev.h compiled for the host (tests/spei_probe) against the
golden within 8 x the restatement's error (spei_cases), with the subtrahend and a table handed back in; the mirror property of
the signed fit; the rank-by-counting of the kernel against std::sort in a stand-alone sanitized program; the [DroughtIndex]
section with the new values, its new refusals, each by its key, and the name of the log-logistic tables; the C-ABI entry in the
header, the library and the bindings."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sindex_np
import spei_cases as cases
import spei_np
from xanthos_amd import ConfigReader, ValidationException, _hip, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PROBE_DIR = os.path.join(ROOT, 'tests', 'spei_probe')
NM = 48
P = ctypes.c_void_p


def ptr(a):
    return None if a is None else a.ctypes.data_as(P)


@pytest.fixture(scope='module')
def probe():
    """tests/spei_probe/libspei_probe.so and rank_check (build() makes them; made here when the suite runs without build())."""
    path = os.path.join(PROBE_DIR, 'libspei_probe.so')
    if not os.path.isfile(path) or not os.path.isfile(os.path.join(PROBE_DIR, 'rank_check')):
        subprocess.run(['make', '-C', PROBE_DIR], check=True, capture_output=True)
    return ctypes.CDLL(path)


def host_index(probe, x, k, ref0, nyr, minus=None, par_in=None, max_shape=cases.MAX_SHAPE):
    x = np.ascontiguousarray(x, dtype=np.float64)
    minus = None if minus is None else np.ascontiguousarray(minus, dtype=np.float64)
    par_in = None if par_in is None else np.ascontiguousarray(par_in, dtype=np.float64)
    idx, par = np.full(x.shape, -7.0), np.full((x.shape[0], 12, 4), -7.0)
    probe.sp_std_index(ctypes.c_int64(x.shape[0]), x.shape[1], k, ref0, nyr, ctypes.c_double(max_shape), ptr(x), ptr(minus),
                       ptr(par_in), ptr(par), ptr(idx))
    return idx, par


def host_fit(probe, s, max_shape=1000.0):
    s = np.ascontiguousarray(s, dtype=np.float64)
    out, srt = np.empty(4), np.empty(max(s.size, 1))
    probe.sp_fit(s.size, ptr(s), ctypes.c_double(max_shape), ptr(out), ptr(srt))
    return out, srt[:s.size]


def host_cdf(probe, X, par):
    X, par = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(par, dtype=np.float64)
    H, idx = np.empty_like(X), np.empty_like(X)
    probe.sp_cdf(ctypes.c_int64(X.size), ptr(X), ptr(par), ptr(H), ptr(idx))
    return H, idx


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ------------------------------------------------------------------ restatement and host build against the golden
@pytest.mark.parametrize('n', cases.INPUTS)
def test_restatement_against_golden(n):
    """The restatement is held to the error measured for it (spei_cases.MEASURED); 8 x that is everyone else's bound."""
    for k in cases.SCALES:
        idx, par = cases.restated(n, k)
        cases.check_against_gold(idx, n, k, 1.0, 'restatement')
        cases.check_parameters(par, n, k, 'restatement')


def test_golden_inputs_hold_the_special_rows():
    assert os.path.getsize(os.path.join(cases.GOLDEN, 'spei.npz')) <= os.path.getsize(os.path.join(cases.GOLDEN, 'sindex.npz'))
    for n in cases.INPUTS:
        x, ref0, nyr = cases.inputs(n)
        after = ref0 + 12 * nyr
        assert x.shape == (cases.NCELL, n) and ref0 % 12 == 0 and after < n
        assert (x[0] < 0).mean() > 0.2 and (x[0] > 0).mean() > 0.2                 # a water balance: both signs
        assert 0.25 < (x[3] == 0).mean() < 0.45 and (x[3] >= 0).all() and np.abs(x[5]).max() < 0.1
        assert (x[6] == 2.5).all() and np.isnan(x[10]).sum() == 1 and x[12].min() > 9e5
        assert np.unique(x[11]).size <= 20 and (x[11] == np.round(x[11])).all()
        par, g = cases.gold_par(n, 1), cases.gold(n, 1)
        assert np.isnan(par[[6, 8]]).all() and np.isnan(g[[6, 8]]).all()          # constant; symmetric: |beta| > max_shape
        month = (n // 3 + 1) % 12                                                  # the NaN's calendar month
        assert np.isnan(par[10, month]).all() and np.isnan(g[10, month::12]).all() and np.isnan(g[10]).sum() == n // 12
        assert (par[7, :, 1] < 0).sum() > 6 and (par[0, :, 1] > 0).sum() > 6       # both signs of the skew ...
        assert (par[7, :, 0] * par[7, :, 1] > 0).all()                             # ... and alpha carries beta's
        big = np.concatenate([np.abs(cases.gold_par(n, k)[[9, 15], :, 1]).ravel() for k in cases.SCALES])
        assert np.nanmax(big) > 100                                                # near-symmetric rows: large |beta|
        # outside the fitted support on either side: exactly -+3.09
        assert (g[13, after:] == -sindex_np.CLIP).mean() > 0.7 and (g[14, after:] == sindex_np.CLIP).mean() > 0.7
        for k in cases.SCALES:                                                     # what the generator asserts
            b = np.abs(cases.gold_par(n, k)[..., 1])
            b = b[~np.isnan(b)]
            assert (np.abs(b - 1) > 1e-6).all() and (np.abs(b / cases.MAX_SHAPE - 1) > 1e-6).all()
            near = np.abs(np.abs(cases.gold(n, k)) - sindex_np.CLIP)
            assert not ((near > 0) & (near < 1e-6)).any() and 8 * cases.MEASURED[(n, k)] < 1e-6
    # the short input's reference period: three years behind month 23 in every calendar month but December
    p24 = cases.gold_par(72, 24)
    assert np.isnan(p24[:, :11]).all() and (p24[:, 11, 3][~np.isnan(p24[:, 11, 3])] == 4).all() and not np.isnan(p24[:, 11]).all()


@pytest.mark.parametrize('n', cases.INPUTS)
def test_host_build_of_the_header_against_golden(probe, n):
    x, ref0, nyr = cases.inputs(n)
    rng = np.random.default_rng(n)
    for k in cases.SCALES:
        idx, par = host_index(probe, x, k, ref0, nyr)
        cases.check_against_gold(idx, n, k, cases.FACTOR, 'host build')
        cases.check_parameters(par, n, k, 'host build')
        # the fit of the restatement: the same operations in the same order
        ref = cases.restated(n, k)[1]
        ok = ~np.isnan(ref).any(-1)
        assert np.allclose(par[ok], ref[ok], rtol=1e-13, atol=0)
        # the table handed back in: the same bits
        again, _ = host_index(probe, x, k, ref0, nyr, par_in=par)
        assert same_bits(again, idx)
        # a subtrahend: x = (x + y) - y exactly when y is a multiple of a power of two far above x's last bit
        y = np.round(rng.uniform(-4, 4, x.shape) * 8) / 8
        sub, _ = host_index(probe, x + y, k, ref0, nyr, minus=y)
        direct, _ = host_index(probe, (x + y) - y, k, ref0, nyr)
        assert same_bits(sub, direct)


def test_fit_of_one_sample(probe):
    rng = np.random.default_rng(7)
    s = rng.gamma(2.0, 3.0, 30) - 4.0
    got, srt = host_fit(probe, s)
    ref = np.array(spei_np.fit_sample(s))
    assert np.array_equal(srt, np.sort(s)) and got[3] == 30 and got[1] > 1 and got[0] > 0
    assert np.allclose(got, ref, rtol=1e-13, atol=0)
    mirrored, _ = host_fit(probe, -s)
    assert mirrored[1] < -1 and mirrored[0] < 0 and np.allclose(mirrored[:3], -got[:3], rtol=1e-9, atol=0)
    assert np.isnan(host_fit(probe, np.append(s, np.nan))[0]).all()
    assert np.isnan(host_fit(probe, [1.0, 2.0, 4.0])[0]).all() and not np.isnan(host_fit(probe, [1.0, 2.0, 4.0, 9.0])[0]).any()      # n < 4
    for c in (0.0, 2.5, 0.1, -1e6):
        assert np.isnan(host_fit(probe, [c] * 9)[0]).all()                                        # constant: 0 / 0
    assert np.isnan(host_fit(probe, [])[0]).all()
    sym = np.array([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]) + 10.0
    assert np.isnan(host_fit(probe, sym)[0]).all()                                                # no skew: |beta| beyond max_shape
    near = np.append(sym, 10.002)
    p = host_fit(probe, near)[0]
    assert np.isnan(p).all() and 1000 < abs(host_fit(probe, near, 1e6)[0][1]) < 1e6
    flat = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 100.0])                                             # |beta| <= 1: unusable
    assert np.isnan(host_fit(probe, flat * 0 + [0, 0, 0, 0, 0, 1.0])[0]).all()
    # the distribution function: outside the support, NaN, and the formula
    H, idx = host_cdf(probe, [got[2] - 1.0, got[2], np.nan, got[2] + got[0]], got)
    assert H[0] == 0.0 and H[1] == 0.0 and idx[0] == -3.09 and np.isnan(H[2]) and np.isnan(idx[2]) and H[3] == 0.5 and idx[3] == 0.0
    H, idx = host_cdf(probe, [mirrored[2] + 1.0, mirrored[2], mirrored[2] + mirrored[0]], mirrored)
    assert H[0] == 1.0 and H[1] == 1.0 and idx[0] == 3.09 and H[2] == 0.5
    assert np.isnan(host_cdf(probe, [1.0], [np.nan] * 4)[0]).all()
    X = np.linspace(s.min() - 1, s.max() + 5, 200)
    H, idx = host_cdf(probe, X, got)
    assert (np.diff(H) >= 0).all() and np.allclose(H, spei_np.cdf(X, *got[:3]), rtol=1e-13, atol=1e-300)


def test_mirror_property(probe):
    """H of the fit to R at x plus H of the fit to -R at -x is 1: the signed formulas describe the mirrored distribution.  Over
    6,000 random samples of n = 4 .. 30 (skewed, near-symmetric, tied).  Bound: 8 x 1.3e-12, the figure of the 20,000-sample CPU
    study behind the definition (two float64 evaluations of one function; measured here 4.8e-14).  A sample whose |beta| lies
    within 1e-6 of 1 is left out, as is one unusable on either side (the rule of the golden generator: all
    values but one equal gives |beta| = 1 exactly, 1 + 1e-14 in doubles, and a 'distribution' that is a point)."""
    rng = np.random.default_rng(1)
    worst, used, unusable = 0.0, 0, 0
    for i in range(6000):
        n = int(rng.integers(4, 31))
        s = (rng.gamma(2.0, 3.0, n) - 4.0, rng.standard_normal(n), np.round(rng.gamma(2.0, 2.0, n)))[i % 3]
        a, b = host_fit(probe, s)[0], host_fit(probe, -s)[0]
        if np.isnan(a).any() or np.isnan(b).any() or abs(abs(a[1]) - 1) <= 1e-6:
            unusable += 1
            continue
        assert a[1] * b[1] < 0
        x = np.concatenate([s, rng.uniform(s.min() - 3, s.max() + 3, 8)])
        e = float(np.abs(host_cdf(probe, x, a)[0] + host_cdf(probe, -x, b)[0] - 1.0).max())
        worst, used = max(worst, e), used + 1
    print('mirror property: max |H + H_mirror - 1| {:.3g} over {} samples ({} unusable)'.format(worst, used, unusable))
    assert used > 5000 and worst <= 8 * 1.3e-12


def test_rank_by_counting_against_std_sort_under_sanitizers(probe):
    """xh_si_rank, the function the kernel ranks with, in a stand-alone program of its own (tests/spei_probe/rank_check.cpp,
    -fsanitize=address,undefined), started as a child process: samples of up to 341 values with ties, signed zeros,
    infinities and NaNs, read at the kernel's stride; the ranks a permutation, the scatter equal to std::sort."""
    out = subprocess.run([os.path.join(PROBE_DIR, 'rank_check'), '1500', '20251'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and '1500 cases, 0 failed' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ------------------------------------------------------------------ the section
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('spei_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = synth.make_forcing(w, NM, seed=50)
    plain = synth.write_example(root, w, f, 1971, 1974, runoff_spinup=25, routing_spinup=6)
    ini = synth.write_example(root, w, f, 1971, 1974, runoff_spinup=25, routing_spinup=6, project='with_spei',
                              drought_index=dict(index_var='balance', scales=(1, 3, 12), distribution='loglogistic'))
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
    assert '[DroughtIndex]' in msg and all(k in msg for k in keys), msg
    return msg


def test_section_takes_the_new_values(tree, tmp_path):
    root, w, f, plain, ini = tree
    from xanthos_amd.drought import standardized
    c = ConfigReader(ini)
    assert c.drought_index == {'var': 'balance', 'scales': [1, 3, 12], 'distribution': 'loglogistic', 'reference_start_year': 1971,
                               'reference_end_year': 1974, 'max_shape': 1000.0, 'parameters': None}
    c = ConfigReader(edited(ini, tmp_path, (r'index_var = balance', 'index_var = Precip'), (r'distribution = loglogistic',
                                                                                           'distribution = Gamma')))
    assert c.drought_index['var'] == 'precip' and c.drought_index['distribution'] == 'gamma'
    for var, dist in (('q', 'loglogistic'), ('soilmoisture', 'loglogistic'), ('avgchflow', 'loglogistic'), ('balance', 'empirical')):
        c = ConfigReader(edited(ini, tmp_path, (r'index_var = balance', 'index_var = ' + var),
                                (r'distribution = loglogistic', 'distribution = ' + dist)))
        assert (c.drought_index['var'], c.drought_index['distribution']) == (var, dist)
    assert standardized.INDEX_NAMES['precip'] == 'SPI' and standardized.INDEX_NAMES['balance'] == 'SPEI'
    assert os.path.basename(standardized.ll_parameter_file(c, 'balance', 12)) == 'drought_index_balance_12m_llparameters_with_spei.npy'
    assert os.path.basename(standardized.parameter_file(c, 'precip', 3)) == 'drought_index_precip_3m_parameters_with_spei.npy'
    # the default dict of a section that names none of the new values is what it was
    c = ConfigReader(edited(ini, tmp_path, (r'index_var = balance', 'index_var = q'), (r'distribution = loglogistic\n', '')))
    assert c.drought_index == {'var': 'q', 'scales': [1, 3, 12], 'distribution': 'gamma', 'reference_start_year': 1971,
                               'reference_end_year': 1974, 'max_shape': 1000.0, 'parameters': None}


def test_new_refusals_name_their_key(tree, tmp_path):
    root, w, f, plain, ini = tree
    no_runoff = ((r'(?s)\[Runoff\].*?\n\[Routing\]', '[Routing]'), (r'(?s)\[Routing\].*?\n\[DroughtIndex\]', '[DroughtIndex]'))
    for var in ('precip', 'balance'):
        msg = refused(edited(ini, tmp_path, (r'index_var = balance', 'index_var = ' + var), *no_runoff), 'index_var', var)
        assert 'runoff_module' in msg
    # balance without a PET module: PET from a file
    pet_file = os.path.join(root, 'pet.npy')
    np.save(pet_file, np.ones((w.ncell, NM)))
    msg = refused(edited(ini, tmp_path, (r'(?s)\[PET\].*?\n\[Runoff\]', '[PET]\npet_module = none\npet_file = {}\n\n[Runoff]'.format(
        pet_file))), 'index_var', 'balance')
    assert 'pet_module' in msg
    refused(edited(ini, tmp_path, (r'distribution = loglogistic', 'distribution = pearson3')), 'distribution', 'pearson3', 'loglogistic')
    refused(edited(ini, tmp_path, (r'index_var = balance', 'index_var = pet')), 'index_var', 'pet', 'balance')
    # parameters: the tables of a log-logistic fit have a name of their own; a gamma table is never read in their place
    stem = os.path.join(str(tmp_path), 'hist', 'historic')
    os.makedirs(os.path.dirname(stem))
    for k in (1, 3, 12):
        np.save(os.path.join(str(tmp_path), 'hist', 'drought_index_balance_{}m_parameters_historic.npy'.format(k)), np.zeros((60, 12, 4)))
    with_par = edited(ini, tmp_path, (r'index_var = balance', 'index_var = balance\nparameters = ' + stem))
    refused(with_par, 'parameters', 'drought_index_balance_1m_llparameters_historic.npy')
    for k in (1, 3):
        np.save(os.path.join(str(tmp_path), 'hist', 'drought_index_balance_{}m_llparameters_historic.npy'.format(k)), np.zeros((60, 12, 4)))
    np.save(os.path.join(str(tmp_path), 'hist', 'drought_index_balance_12m_llparameters_historic.npy'), np.zeros((60, 12, 3)))
    msg = refused(with_par, 'parameters', '(60, 12, 3)')
    assert '[60, 12, 4]' in msg and 'gamma' in msg
    np.save(os.path.join(str(tmp_path), 'hist', 'drought_index_balance_12m_llparameters_historic.npy'), np.zeros((60, 12, 4)))
    c = ConfigReader(with_par)
    assert sorted(c.drought_index['parameters']) == [1, 3, 12] and c.drought_index['parameters'][3].endswith(
        'drought_index_balance_3m_llparameters_historic.npy')
    # ... and with gamma the same stem still resolves to the gamma tables
    c = ConfigReader(edited(with_par, tmp_path, (r'distribution = loglogistic', 'distribution = gamma'), name='gamma.ini'))
    assert c.drought_index['parameters'][3].endswith('drought_index_balance_3m_parameters_historic.npy')
    refused(edited(with_par, tmp_path, (r'distribution = loglogistic', 'distribution = empirical'), name='emp.ini'), 'parameters', 'empirical')


def test_without_the_section_nothing_changes(tree):
    root, w, f, plain, ini = tree
    base = vars(ConfigReader(plain))
    assert base['CalculateDroughtIndex'] == 0 and base['drought_index'] is None
    assert 'DroughtIndex' not in open(plain).read()


# ------------------------------------------------------------------ the C-ABI entry
def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    assert re.search(r'\bint xh_std_index2\(xh_ctx \*ctx, int64_t ncell, int32_t nmonths, int32_t nscale, const int32_t \*h_scale,', header)
    assert re.search(r'const double \*d_x, const double \*d_minus,\s+const double \*const \*h_d_par_in', header)
    assert re.search(r'#define XH_STD_INDEX_LOGLOGISTIC 2\b', header)
    assert 'xh_std_index2 replaces NO function of the reference' in header
    assert len(_hip.SIGNATURES['xh_std_index2'][1]) == len(_hip.SIGNATURES['xh_std_index'][1]) + 1 == 14
    assert hasattr(_hip.lib(), 'xh_std_index2') and hasattr(_hip.lib(), 'xh_std_index')
    assert _hip.STD_INDEX_DIST2 == {'gamma': 0, 'empirical': 1, 'loglogistic': 2}
    dev = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'xh_sindex_dev.h')).read()
    assert re.search(r'#define XH_SI_LOGLOGISTIC 2\b', dev) and 'exp(beta log z)' in dev and '6 w1 - w0 - 6 w2' in dev


# ------------------------------------------------------------------ where Components takes the precipitation from
def test_precipitation_of_a_sharded_run_is_refused_by_key():
    """The root of a sharded run holds the gathered outputs, and no rank the whole forcing: index_var = precip / balance is
    refused by key rather than indexed in part.  A run that went stage by stage has no pipeline: the loader's host array."""
    from types import SimpleNamespace
    from xanthos_amd.components import Components
    s = SimpleNamespace(ncell=60, nmonths=NM)
    host = np.ones((60, NM))
    staged = SimpleNamespace(pipe=None, s=s, data=SimpleNamespace(precip=host))
    assert Components._precipitation(staged, 'precip') is host
    whole = SimpleNamespace(pipe=SimpleNamespace(forcing={'precip': SimpleNamespace(shape=(60, NM))}), s=s, data=None)
    assert Components._precipitation(whole, 'balance') is whole.pipe.forcing['precip']
    root = SimpleNamespace(pipe=SimpleNamespace(out={}, plan=None, ncell=60, nmonths=NM), s=s, data=None)      # (as simulation() leaves it)
    part = SimpleNamespace(pipe=SimpleNamespace(forcing={'precip': SimpleNamespace(shape=(31, NM))}), s=s, data=None)
    for c in (root, part):
        for var in ('precip', 'balance'):
            with pytest.raises(ValidationException) as exc:
                Components._precipitation(c, var)
            assert '[DroughtIndex]' in str(exc.value) and 'index_var = ' + var in str(exc.value) and 'sharded' in str(exc.value)


def test_schedule_keeps_a_forcing_set_until_its_write_out_has_read_it():
    """With SPI / SPEI the write-out of member k reads the forcing set that member k + 2 uploads into: run_schedule's
    ``write_reads_forcing`` makes that upload wait for the write-out too (and otherwise, as before, for the compute alone)."""
    import threading
    from xanthos_amd import ensemble
    for flag in (True, False):
        log, lock = [], threading.Lock()

        def stage(name):
            def run(k, i):
                with lock:
                    log.append((name + ' begins', k, i))
                    log.append((name + ' ends', k, i))
            return run
        ensemble.run_schedule(6, stage('upload'), stage('compute'), stage('write'), overlap=True, write_reads_forcing=flag)
        at = {e: n for n, e in enumerate(log)}
        assert len(log) == 36
        for k in range(2, 6):
            assert at[('upload begins', k, k % 2)] > at[('compute ends', k - 2, k % 2)]
            assert at[('compute begins', k, k % 2)] > at[('write ends', k - 2, k % 2)]
            if flag:
                assert at[('upload begins', k, k % 2)] > at[('write ends', k - 2, k % 2)]
