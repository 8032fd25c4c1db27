"""CPU checks of the standardized drought indices: the numpy / scipy restatement (sindex_np) against the 40-digit golden; the
functions of csrc/xh_sindex_dev.h compiled for the host (tests/sindex_probe) -- P(a, x) and ndtri against mpmath, the loop
bound, the fit and the evaluation against the golden within 8 x the restatement's error (sindex_cases) --; the empirical rank
formula against brute-force counts; the [DroughtIndex] section and its refusals, each by its key; the ensemble plan with
index<k>; the C-ABI entry in the header, the library and the bindings."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sindex_cases as cases
import sindex_np
from xanthos_amd import ConfigReader, ValidationException, _hip, ensemble, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PROBE_DIR = os.path.join(ROOT, 'tests', 'sindex_probe')
NM = 48
P = ctypes.c_void_p


def ptr(a):
    return None if a is None else a.ctypes.data_as(P)


@pytest.fixture(scope='module')
def probe():
    """tests/sindex_probe/libsindex_probe.so (build() makes it; made here when the suite runs without build())."""
    path = os.path.join(PROBE_DIR, 'libsindex_probe.so')
    if not os.path.isfile(path):
        subprocess.run(['make', '-C', PROBE_DIR], check=True)
    return ctypes.CDLL(path)


def host_index(probe, x, k, ref0, nyr, dist, par_in=None, max_shape=cases.MAX_SHAPE):
    x = np.ascontiguousarray(x, dtype=np.float64)
    idx, par, X = np.full(x.shape, -7.0), np.full((x.shape[0], 12, 4), -7.0), np.full(x.shape, -7.0)
    par_in = None if par_in is None else np.ascontiguousarray(par_in, dtype=np.float64)
    probe.si_std_index(ctypes.c_int64(x.shape[0]), x.shape[1], k, ref0, nyr, cases.DISTS.index(dist), ctypes.c_double(max_shape),
                       ptr(x), ptr(par_in), ptr(par), ptr(X), ptr(idx))
    return idx, par, X


# ------------------------------------------------------------------ restatement and host build against the golden
@pytest.mark.parametrize('dist', cases.DISTS)
@pytest.mark.parametrize('n', cases.INPUTS)
def test_restatement_against_golden(n, dist):
    """The restatement is held to the error measured for it (sindex_cases.MEASURED); 8 x that is everyone else's bound."""
    for k in cases.SCALES:
        cases.check_against_gold(cases.restated(n, dist, k)[0], n, dist, k, cases.MEASURED[(n, dist, k)], 'restatement')


def test_golden_inputs_hold_the_special_rows():
    for n in cases.INPUTS:
        x, ref0, nyr = cases.inputs(n)
        assert x.shape == (70, n) and ref0 % 12 == 0 and ref0 + 12 * nyr <= n
        assert (x[6] == 0).all() and np.isnan(x[10]).sum() == 1 and (x[11] < 0).sum() == 1
        assert 0.25 < (x[3] == 0).mean() < 0.45 and x[5].max() < 0.1
        assert ((x[7].reshape(-1, 12) > 0).sum(0) == 3).all()
        par = cases.restated(n, 'gamma', 1)[1]
        assert np.isnan(par[[6, 7, 8]]).all()                              # all zero, 3 positives, alpha > max_shape
        for row, month in ((10, (n // 3 + 1) % 12), (11, (n // 2 + 5) % 12)):     # the NaN's / the negative value's calendar month
            assert np.isnan(par[row, month]).all() and not np.isnan(np.delete(par[row], month, 0)).any()
        assert 150 < np.nanmin(par[9, :, 1]) and np.nanmax(par[12, :, 1]) < cases.MAX_SHAPE
        g = cases.gold(n, 'gamma', 1)
        assert np.isnan(g[[6, 7, 8]]).all() and not np.isnan(g[0]).any()
        assert np.isnan(g[11, (n // 2 + 5) % 12::12]).all() and np.isnan(g[11]).sum() == n // 12
    # months outside the sub-period reference: values beyond every sample are clipped
    g = cases.gold(360, 'gamma', 1)
    assert (np.abs(g[:, :60][~np.isnan(g[:, :60])]) == sindex_np.CLIP).any()


@pytest.mark.parametrize('dist', cases.DISTS)
@pytest.mark.parametrize('n', cases.INPUTS)
def test_host_build_of_the_header_against_golden(probe, n, dist):
    x, ref0, nyr = cases.inputs(n)
    for k in cases.SCALES:
        idx, par, X = host_index(probe, x, k, ref0, nyr, dist)
        assert np.array_equal(X.view(np.uint64), sindex_np.accumulate(x, k).view(np.uint64))       # the sum, left to right
        cases.check_against_gold(idx, n, dist, k, cases.bound(n, dist, k), 'host build')
        if dist == 'empirical':
            assert (par == -7.0).all()
            continue
        ref = cases.restated(n, dist, k)[1]
        nan_rows = np.isnan(ref).any(-1)
        assert np.array_equal(np.isnan(par), np.repeat(nan_rows[..., None], 4, -1))
        ok = ~nan_rows
        assert np.array_equal(par[ok][:, 0], ref[ok][:, 0]) and np.array_equal(par[ok][:, 3], ref[ok][:, 3])
        assert np.allclose(par[ok][:, 1:3], ref[ok][:, 1:3], rtol=1e-9, atol=0)
        # the table handed back in: the same bits
        again, _, _ = host_index(probe, x, k, ref0, nyr, dist, par_in=par)
        assert np.array_equal(again.view(np.uint64), idx.view(np.uint64))


def test_fit_of_one_sample(probe):
    def fit(s, max_shape=1000.0):
        s = np.ascontiguousarray(s, dtype=np.float64)
        out = np.empty(4)
        probe.si_fit_gamma(s.size, ptr(s), ctypes.c_double(max_shape), ptr(out))
        return out
    rng = np.random.default_rng(7)
    s = rng.gamma(2.0, 3.0, 30)
    s[[2, 9, 20]] = 0.0
    got, ref = fit(s), np.array(sindex_np.fit_gamma_sample(s))
    assert got[0] == 0.1 and got[3] == 30 and np.allclose(got, ref, rtol=1e-13, atol=0)
    assert np.isnan(fit(np.append(s, np.nan))).all() and np.isnan(fit(np.append(s, -1e-300))).all()
    assert np.isnan(fit([0, 0, 1.0, 2.0, 3.0])).all() and not np.isnan(fit([0, 0, 1.0, 2.0, 3.0, 4.0])).any()      # np < 4
    assert np.isnan(fit([2.0] * 8)).all()                                                     # A = 0: no spread
    near = 100.0 * (1 + 1e-3 * rng.standard_normal(40))
    assert np.isnan(fit(near)).all() and not np.isnan(fit(near, 1e7)).any()                   # alpha ~ 1e6 > max_shape
    assert np.isnan(fit([])).all()


# ------------------------------------------------------------------ P(a, x) and ndtri against mpmath
def test_incomplete_gamma_against_mpmath_and_the_loop_bound(probe):
    """a in [0.01, 1000] x (x / a) in [1e-3, 10], and x next to the switch a + 1 between the series and the continued fraction.
    Every call converges inside XH_SI_MAXIT = 512: measured here, at most 269 iterations of the series (a = 1000, x just
    below a + 1; the header derives 312) and 90 of the continued fraction.
    Error, relative, on whichever of P and Q = 1 - P the function computes directly: that value is exp(E) times a sum of
    positive terms (or a continued fraction) good to a few eps.  For a >= 12, E = a (log1p(u) - u) - c(a) is of the size of
    |ln value| + O(ln a) and carries a handful of roundings: eps (16 + 8 |ln value|), eps = 2^-52.  For a < 12, E = a log x - x
    - lgamma(a) with lgamma from Stirling's form at z = a + N in [12, 13): its parts (z - 1/2) log z <= 32, z <= 13 and the
    logarithm of a (a + 1) ... (a + N - 1) <= 18 are each rounded, which adds up to 64 eps.  Held to that where the value is
    above 1e-200 (measured: 27 eps at a = 0.075); in absolute terms on P <= 1 that is at most 83 eps = 1.9e-14 (measured 5.7e-15,
    scipy's own 1.0e-15): an index moves by dP / phi(z), 5e-14 at the centre, for that.  The golden tests hold the index
    itself to its bound."""
    import mpmath as mp
    mp.mp.dps = 40
    a = 10.0 ** np.linspace(-2, 3, 41)
    r = 10.0 ** np.linspace(-3, 1, 33)
    A, R = [v.ravel() for v in np.meshgrid(a, r)]
    A = np.concatenate([A, a, a, a])
    X = np.concatenate([A[:a.size * r.size] * R, a + 1.0, np.nextafter(a + 1.0, 0.0), np.nextafter(a + 1.0, 1e9)])
    got, its = np.empty_like(A), np.empty(A.size, dtype=np.int32)
    probe.si_gammap(ctypes.c_int64(A.size), ptr(A), ptr(X), ptr(got), ptr(its))
    assert probe.si_maxit() == 512
    series = X < A + 1.0
    print('iterations: series max {}, continued fraction max {}'.format(its[series].max(), its[~series].max()))
    assert its.max() <= 512 and not np.isnan(got).any()          # (0: Q underflows, no loop)
    assert its[series].max() <= 312
    p = np.array([float(mp.gammainc(mp.mpf(u), 0, mp.mpf(v), regularized=True)) for u, v in zip(A, X)])
    q = np.array([float(mp.gammainc(mp.mpf(u), mp.mpf(v), mp.inf, regularized=True)) for u, v in zip(A, X)])
    print('max |P - mp| {:.3g}'.format(np.abs(got - p).max()))
    assert np.abs(got - p).max() <= 83 * 2.0 ** -52
    eps = 2.0 ** -52
    s = series & (p > 1e-200)
    rel = np.abs(got[s] - p[s]) / (p[s] * eps * (16 + 8 * np.abs(np.log(p[s])) + 64 * (A[s] < 12)))
    print('series: max error / bound {:.3g}'.format(rel.max()))
    assert rel.max() <= 1.0
    c = ~series & (q > 1e-3)                                     # (1 - P as a double resolves Q only to 1.1e-16 absolute)
    rel = (np.abs((1.0 - got[c]) - q[c]) - 1.2e-16) / (q[c] * eps * (16 + 8 * np.abs(np.log(q[c])) + 64 * (A[c] < 12)))
    print('continued fraction: max error / bound {:.3g}'.format(rel.max()))
    assert rel.max() <= 1.0
    # arguments outside the domain, the ends
    edge_a = np.array([1.0, 1.0, -1.0, 0.0, np.nan, 2.0, 2.0, np.inf])
    edge_x = np.array([0.0, np.inf, 1.0, 1.0, 1.0, -1.0, np.nan, 1.0])
    out, it = np.empty(8), np.empty(8, dtype=np.int32)
    probe.si_gammap(ctypes.c_int64(8), ptr(edge_a), ptr(edge_x), ptr(out), ptr(it))
    assert out[0] == 0.0 and out[1] == 1.0 and np.isnan(out[2:]).all()
    # beyond the design limit the bound may be met: NaN, never a spin
    big_a, big_x = np.array([4e5]), np.array([4e5])
    probe.si_gammap(ctypes.c_int64(1), ptr(big_a), ptr(big_x), ptr(out), ptr(it))
    assert np.isnan(out[0]) and it[0] == 513


def test_ndtri_against_mpmath(probe):
    """p from 1e-300 to 1 - 1e-16, with both region boundaries (|p - 1/2| = 0.425; r = sqrt(-log p) = 5, p = exp(-25)) and their
    neighbours.  AS 241's rational functions are good to about 1e-16 relative; their evaluation in doubles adds the rounding
    of two degree-7 Horner forms of positive terms (<= 2 ulp each), the division, and in the tails one ulp of r = sqrt(-log p)
    carried through a function of logarithmic slope 1 - 2: held to 5 ulp = 1.2e-15 of the value (measured 7.5e-16, at p =
    1e-179; scipy's ndtri 4.7e-16 on the same points)."""
    import mpmath as mp
    mp.mp.dps = 40
    e25 = float(mp.exp(-25))
    p = np.concatenate([10.0 ** np.linspace(-300, -1, 300), np.linspace(0.01, 0.99, 491), 1.0 - 10.0 ** np.linspace(-16, -1, 151),
                        [0.075, np.nextafter(0.075, 0), np.nextafter(0.075, 1), 0.925, np.nextafter(0.925, 0),
                         np.nextafter(0.925, 1), e25, np.nextafter(e25, 0), np.nextafter(e25, 1), 0.5, 1e-3, 1 - 1e-3]])
    got = np.empty_like(p)
    probe.si_ndtri(ctypes.c_int64(p.size), ptr(p), ptr(got))
    def exact(v, start):
        if v < 1e-5:                   # (2 p - 1 would need 300 digits: solve log Phi(z) = log p from the value under test)
            return float(mp.findroot(lambda z: mp.log(mp.ncdf(z)) - mp.log(mp.mpf(v)), mp.mpf(start)))
        return float(mp.sqrt(2) * mp.erfinv(2 * mp.mpf(v) - 1))
    ref = np.array([exact(float(v), float(g)) for v, g in zip(p, got)])
    err = np.abs(got - ref) / np.where(ref == 0, 1.0, np.abs(ref))
    err[ref == 0] = np.abs(got[ref == 0])
    print('ndtri: max relative error {:.3g}'.format(err.max()))
    assert err.max() <= 1.2e-15 and got[p == 0.5][0] == 0.0
    ends = np.array([0.0, 1.0, -0.5, 1.5, np.nan])
    out = np.empty(5)
    probe.si_ndtri(ctypes.c_int64(5), ptr(ends), ptr(out))
    assert out[0] == -np.inf and out[1] == np.inf and out[2] == -np.inf and out[3] == np.inf and np.isnan(out[4])


# ------------------------------------------------------------------ the empirical rank formula
def test_empirical_rank_on_ties_and_outside_values(probe):
    from scipy.special import ndtri
    sample = np.array([3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 6.0, 5.0, 3.0, 5.0])
    X = np.array([5.0, 1.0, 9.0, 0.5, 10.0, 3.5, 3.0, np.nan])
    for in_ref in (0, 1):
        flags = np.full(X.size, in_ref, dtype=np.int32)
        got = np.empty_like(X)
        probe.si_eval_empirical(ctypes.c_int64(X.size), ptr(X), ptr(flags), sample.size, ptr(sample), ptr(got))
        for xv, g in zip(X, got):
            if np.isnan(xv):
                assert np.isnan(g)
                continue
            # brute force: merge X into the sample unless it is in it already, rank = mean of its tied positions
            merged = np.sort(sample if in_ref else np.append(sample, xv))
            if in_ref and xv not in sample:
                continue                                   # (in = 1 says X is an element of the sample)
            pos = np.flatnonzero(merged == xv) + 1
            p = (pos.mean() - 0.44) / (merged.size + 0.12)
            assert abs(g - np.clip(ndtri(p), -3.09, 3.09)) <= 4e-16 * max(1.0, abs(g)), (xv, in_ref)
            assert g == np.clip(ndtri(sindex_np.empirical_position(xv, sample, in_ref)), -3.09, 3.09) or \
                abs(g - ndtri(sindex_np.empirical_position(xv, sample, in_ref))) <= 9e-16
    # below / above every element of the sample, a sample of three, a NaN in the sample
    flags = np.zeros(2, dtype=np.int32)
    got = np.empty(2)
    probe.si_eval_empirical(ctypes.c_int64(2), ptr(np.array([0.0, 99.0])), ptr(flags), sample.size, ptr(sample), ptr(got))
    assert abs(got[0] + got[1]) <= 4e-15 and abs(got[1] - ndtri((12 - 0.44) / 12.12)) <= 9e-16
    probe.si_eval_empirical(ctypes.c_int64(2), ptr(np.array([0.0, 99.0])), ptr(flags), 3, ptr(sample), ptr(got))
    assert np.isnan(got).all()
    bad = sample.copy()
    bad[4] = np.nan
    probe.si_eval_empirical(ctypes.c_int64(2), ptr(np.array([0.0, 99.0])), ptr(flags), bad.size, ptr(bad), ptr(got))
    assert np.isnan(got).all()


# ------------------------------------------------------------------ the section
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('sindex_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = synth.make_forcing(w, NM, seed=50)
    plain = synth.write_example(root, w, f, 1971, 1974, runoff_spinup=25, routing_spinup=6)
    text = open(plain).read()
    ini = synth.write_example(root, w, f, 1971, 1974, runoff_spinup=25, routing_spinup=6, project='with_index',
                              drought_index=dict(index_var='q', scales=(1, 3, 12)))
    return root, w, f, plain, text, ini


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


def test_section_is_parsed_and_defaults(tree, tmp_path):
    root, w, f, plain, text, ini = tree
    c = ConfigReader(ini)
    assert c.CalculateDroughtIndex == 1
    assert c.drought_index == {'var': 'q', 'scales': [1, 3, 12], 'distribution': 'gamma', 'reference_start_year': 1971,
                               'reference_end_year': 1974, 'max_shape': 1000.0, 'parameters': None}
    c = ConfigReader(edited(ini, tmp_path, (r'index_var = q', 'index_var = AvgChFlow\ndistribution = Empirical\n'
                                            'reference_start_year = 1972\nreference_end_year = 1973\nmax_shape = 50')))
    assert c.drought_index['var'] == 'avgchflow' and c.drought_index['distribution'] == 'empirical'
    assert (c.drought_index['reference_start_year'], c.drought_index['reference_end_year']) == (1972, 1973)
    assert c.drought_index['max_shape'] == 50.0
    from xanthos_amd.drought import standardized
    assert standardized.reference_window(c) == (12, 2)
    assert os.path.basename(standardized.output_stem(c, 'avgchflow', 3)) == 'drought_index_avgchflow_3m_with_index'
    assert os.path.basename(standardized.parameter_file(c, 'q', 12)) == 'drought_index_q_12m_parameters_with_index.npy'


def test_without_the_flag_nothing_changes(tree, tmp_path):
    root, w, f, plain, text, ini = tree
    # the example writers' default text is what it was: no flag, no section
    assert 'DroughtIndex' not in text
    again = synth.write_example(str(tmp_path), w, f, 1971, 1974, runoff_spinup=25, routing_spinup=6)
    assert open(again).read().replace(str(tmp_path), root) == text
    base = vars(ConfigReader(plain))
    assert base['CalculateDroughtIndex'] == 0 and base['drought_index'] is None
    # a section without the flag, or the flag at 0, is not read: the same settings, whatever the section holds
    for sub in ((r'CalculateDroughtIndex = 1\n', ''), (r'CalculateDroughtIndex = 1', 'CalculateDroughtIndex = 0')):
        off = edited(ini, tmp_path, sub, (r'index_var = q', 'index_var = nonsense'), (r'ProjectName = with_index',
                                                                                     'ProjectName = pm_abcd_mrtm_synth'))
        got = vars(ConfigReader(off))
        assert set(got) == set(base)
        assert all(np.array_equal(got[k], base[k]) if isinstance(base[k], np.ndarray) else got[k] == base[k] for k in base)
    with pytest.raises(ValidationException, match='CalculateDroughtIndex'):
        ConfigReader(edited(ini, tmp_path, (r'CalculateDroughtIndex = 1', 'CalculateDroughtIndex = 2')))
    with pytest.raises(ValidationException, match=r'no \[DroughtIndex\] section'):
        ConfigReader(edited(ini, tmp_path, (r'(?s)\n\[DroughtIndex\].*', '\n')))


def test_refusals_name_their_key(tree, tmp_path):
    root, w, f, plain, text, ini = tree
    refused(edited(ini, tmp_path, (r'index_var = q', 'index_var = q\nreference_start_year = 1970')), 'reference_start_year', '1970')
    refused(edited(ini, tmp_path, (r'index_var = q', 'index_var = q\nreference_end_year = 1975')), 'reference_end_year', '1975')
    refused(edited(ini, tmp_path, (r'index_var = q', 'index_var = q\nreference_start_year = 1973\nreference_end_year = 1972')),
            'reference_end_year')
    msg = refused(edited(ini, tmp_path, (r'index_var = q', 'index_var = avgchflow'), (r'(?s)\[Routing\].*?\n\[DroughtIndex\]',
                                                                                     '[DroughtIndex]')), 'index_var', 'avgchflow')
    assert 'routing_module' in msg
    refused(edited(ini, tmp_path, (r'index_var = q', 'index_var = pet')), 'index_var', 'pet')
    refused(edited(ini, tmp_path, (r'OutputInYear = 0', 'OutputInYear = 1')), 'OutputInYear')
    refused(edited(ini, tmp_path, (r'index_var = q', 'index_var = q\ndistribution = weibull')), 'distribution', 'weibull')
    for bad in ('0, 3', '1, 49', '3, 3', '1, 2, 3, 4, 5, 6, 7, 8, 9', 'three'):
        refused(edited(ini, tmp_path, (r'scales = 1, 3, 12', 'scales = ' + bad)), 'scales')
    refused(edited(ini, tmp_path, (r'scales = 1, 3, 12\n', '')), 'scales')
    refused(edited(ini, tmp_path, (r'index_var = q', 'index_var = q\nmax_shape = 0')), 'max_shape')
    # parameters: not with empirical; files that are missing or whose shape does not fit
    stem = os.path.join(str(tmp_path), 'hist', 'historic')
    os.makedirs(os.path.dirname(stem))
    refused(edited(ini, tmp_path, (r'index_var = q', 'index_var = q\ndistribution = empirical\nparameters = ' + stem)),
            'parameters', 'empirical')
    with_par = edited(ini, tmp_path, (r'index_var = q', 'index_var = q\nparameters = ' + stem))
    refused(with_par, 'parameters', 'drought_index_q_1m_parameters_historic.npy')
    for k in (1, 3):
        np.save(os.path.join(str(tmp_path), 'hist', 'drought_index_q_{}m_parameters_historic.npy'.format(k)), np.zeros((60, 12, 4)))
    np.save(os.path.join(str(tmp_path), 'hist', 'drought_index_q_12m_parameters_historic.npy'), np.zeros((59, 12, 4)))
    msg = refused(with_par, 'parameters', '(59, 12, 4)')
    assert '[60, 12, 4]' in msg
    np.save(os.path.join(str(tmp_path), 'hist', 'drought_index_q_12m_parameters_historic.npy'), np.zeros((60, 12, 4)))
    c = ConfigReader(with_par)
    assert sorted(c.drought_index['parameters']) == [1, 3, 12] and c.drought_index['parameters'][3].endswith(
        'drought_index_q_3m_parameters_historic.npy')
    # a file name with {k} for the scale
    for k in (1, 3, 12):
        np.save(os.path.join(str(tmp_path), 'hist', 'fit{}.npy'.format(k)), np.zeros((60, 12, 4)))
    c = ConfigReader(edited(ini, tmp_path, (r'index_var = q', 'index_var = q\nparameters = ' +
                                            os.path.join(str(tmp_path), 'hist', 'fit{k}.npy'))))
    assert c.drought_index['parameters'][12].endswith('fit12.npy')


# ------------------------------------------------------------------ the ensemble plan
def test_validate_takes_index_scales_and_counts_their_stack(tree, tmp_path):
    root, w, f, plain, text, ini = tree
    members = [('a', {}), ('b', {}), ('c', {})]
    c = ConfigReader(ini)
    base = ensemble.validate(c, members, statistics=['mean', 'q10'], statistics_vars=['q'])
    plan = ensemble.validate(c, members, statistics=['mean', 'q10'], statistics_vars=['q', 'index3'])
    assert plan.statistics_vars == ['q', 'index3']
    assert plan.bytes_needed == base.bytes_needed + 8 * 60 * NM * 3              # one [ncell, nmonths] array per member
    two = ensemble.validate(c, members, statistics=['mean', 'q10'], statistics_vars=['q', 'index3', 'index12'])
    assert two.bytes_needed == base.bytes_needed + 2 * 8 * 60 * NM * 3
    assert ensemble.validate(c, members, statistics=['mean']).statistics_vars == ['q', 'avgchflow']        # the default: as before
    for bad in ('index6', 'index', 'index03x'):
        with pytest.raises(ValidationException) as exc:
            ensemble.validate(c, members, statistics=['mean'], statistics_vars=['q', bad])
        assert 'statistics_vars' in str(exc.value) and bad in str(exc.value) and 'index3' in str(exc.value)
    with pytest.raises(ValidationException) as exc:                              # no [DroughtIndex]: no index at all
        ensemble.validate(ConfigReader(plain), members, statistics=['mean'], statistics_vars=['index3'])
    assert 'statistics_vars' in str(exc.value) and 'index3' in str(exc.value)
    assert ensemble.index_scale('index12') == 12 and ensemble.index_scale('q') is None
    # member_outputs = 0 with the index's statistics alone is a valid request
    assert ensemble.validate(c, members, statistics=['mean'], statistics_vars=['index1'], member_outputs=0).statistics_vars == ['index1']


# ------------------------------------------------------------------ the C-ABI entry
def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    assert re.search(r'\bint xh_std_index\(xh_ctx \*ctx, int64_t ncell, int32_t nmonths, int32_t nscale, const int32_t \*h_scale,',
                     header)
    assert 'replaces NO function of the reference' in header
    assert 'xh_std_index' in _hip.SIGNATURES and len(_hip.SIGNATURES['xh_std_index'][1]) == 13
    assert hasattr(_hip.lib(), 'xh_std_index') and hasattr(_hip.Context, 'std_index')
    assert _hip.lib().xh_abi_version() == _hip.ABI_VERSION
    assert _hip.STD_INDEX_DIST == {'gamma': 0, 'empirical': 1}
