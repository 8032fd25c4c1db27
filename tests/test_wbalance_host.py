"""Water balance and Budyko signatures per row, everything a machine without a GPU can check: the numpy restatement
(tests/wbalance_np.py) against np.median, np.corrcoef and np.linalg.lstsq, the host build of csrc/xh_wbalance_dev.h
(tests/wbalance_probe) against the restatement, both against 40-digit values, the padded sort and the median against std::sort
under the sanitizers, the [WaterBalance] section's refusals and the C-ABI bookkeeping.

What is bit for bit and what is bounded.  Every column but two is comparisons, +, -, x, / and sqrt in a fixed order: the
restatement, the host build and the device give the same bits.  omega and budyko_dev pass through exp, log, log1p and expm1, which
every build takes from another library.  tests/golden/make_golden_wbalance.py measures how far the restatement lies from 40-digit
values over the 15 kinds of quadruple at the 11 year counts of tests/wbalance_cases.py, with AET and without, per quantity
(relative to the 40-digit value, absolute where that is 0):

    n_years, n_months, lag_peak   0
    p_mean       2.483e-16      pet_mean     2.526e-16      aet_mean     2.507e-16      q_mean       2.866e-16
    runoff_ratio 3.571e-16      aridity      3.559e-16      evaporative  3.596e-16      dry_fraction 7.613e-17
    elast_p      3.135e-11      elast_pet    1.944e-10      elast_p_ls   4.923e-12      elast_pet_ls 1.475e-06
    r_pq         4.614e-13      r_peak       2.818e-16      annual       5.216e-16      xcorr        1.242e-11
    residual, closure           2.495e+02   (a balance that closes but for rounding: the measure is relative to a value near 0)
    omega        2.532e-15      relative to the 40-digit root
    budyko_dev   3.963e-16      relative to max(|budyko_dev|, 1)

(the figures of 1e-11 and larger belong to the quadruple shifted by 1e6, whose deviations cancel six digits, and to nearly
collinear years).  The two bounded columns are held, in every implementation and on every row, to 4 x their figure against the
40-digit value -- the margin because the device's exp, log1p and expm1 are other implementations -- and not below 4 ulp
(4 x 2^-52 of either measure): 1.013e-14 for omega, 1.585e-15 for budyko_dev.  The other columns of the restatement are held to
the 40-digit values by a bound from first-order error propagation, written down at `tolerances`."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import wbalance_cases as cases
import wbalance_np as wnp
from xanthos_amd import ConfigReader, ValidationException, _hip, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PROBE_DIR = os.path.join(ROOT, 'tests', 'wbalance_probe')
P = ctypes.c_void_p
EPS = 2.0 ** -52
BOUNDED = (11, 12)
BIT_COLUMNS = [c for c in range(wnp.NCOL) if c not in BOUNDED]
MEASURED = {'omega': 2.532e-15, 'budyko_dev': 3.963e-16}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def bounded_columns(golden, table, years, with_aet, tag):
    """omega and budyko_dev of ``table`` (the rows of wbalance_cases.rows(years)) against the 40-digit values: every row, none
    left out."""
    g = golden('wbalance')
    dist = g['dist_table']
    assert dist[11] == pytest.approx(MEASURED['omega'], rel=1e-3) and dist[12] == pytest.approx(MEASURED['budyko_dev'], rel=1e-3)
    key = '{}_{}'.format('' if with_aet else '_noaet', years)
    hi, lo = g['table' + key], g['table_lo' + key]
    assert np.array_equal(np.isnan(table[:, BOUNDED]), np.isnan(hi[:, BOUNDED])), tag
    with np.errstate(invalid='ignore'):
        omega = np.abs((table[:, 11] - hi[:, 11]) - lo[:, 11]) / np.abs(hi[:, 11])
        dev = np.abs((table[:, 12] - hi[:, 12]) - lo[:, 12]) / np.maximum(np.abs(hi[:, 12]), 1.0)
    for name, err, measured in (('omega', omega, dist[11]), ('budyko_dev', dev, dist[12])):
        b = max(4.0 * measured, 4.0 * EPS)
        worst = float(np.nanmax(err)) if (~np.isnan(err)).any() else 0.0
        print('{}: {} max error {:.3e}, bound {:.3e}'.format(tag, name, worst, b))
        assert worst <= b, (tag, name, worst, b)


def held(golden, got, ref, years, with_aet, tag):
    """(table, annual, xcorr) of the case rows of ``years`` against the host build's or the restatement's: the same bits in
    every column but two, and those inside their bounds."""
    assert same_bits(got[0][:, BIT_COLUMNS], ref[0][:, BIT_COLUMNS]), tag
    assert same_bits(got[1], ref[1]) and same_bits(got[2], ref[2]), tag
    assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0])), tag
    bounded_columns(golden, got[0], years, with_aet, tag)


@pytest.fixture(scope='module')
def probe():
    """tests/wbalance_probe/libwbalance_probe.so and median_check (build() makes them; made here when the suite runs without
    it)."""
    path = os.path.join(PROBE_DIR, 'libwbalance_probe.so')
    if not os.path.isfile(path) or not os.path.isfile(os.path.join(PROBE_DIR, 'median_check')):
        subprocess.run(['make', '-C', PROBE_DIR], check=True, capture_output=True)
    lib = ctypes.CDLL(path)
    lib.wp_water_balance.restype = ctypes.c_int
    lib.wp_water_balance.argtypes = [ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_double] + [P] * 7
    lib.wp_omega.restype = lib.wp_fu.restype = None
    lib.wp_omega.argtypes = [ctypes.c_int64, P, P, P]
    lib.wp_fu.argtypes = [ctypes.c_int64, P, ctypes.c_double, P]
    return lib


def host_balance(probe, p, pet, q, aet=None, start=0, nyear=None, max_lag=cases.MAX_LAG, omega0=cases.OMEGA0, annual=True, xcorr=True,
                 fill=-777.0):
    arrays = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (p, pet, q, aet)]
    nrows, stride = arrays[0].shape
    nyear = (stride - start) // 12 if nyear is None else nyear
    table = np.full((nrows, wnp.NCOL), fill)
    ann, xc = np.full((nrows, 4, nyear), fill), np.full((nrows, max_lag + 1), fill)
    rc = probe.wp_water_balance(nrows, stride, start, nyear, max_lag, omega0, *[None if a is None else a.ctypes.data_as(P) for a in arrays],
                                table.ctypes.data_as(P), ann.ctypes.data_as(P) if annual else None, xc.ctypes.data_as(P) if xcorr else None)
    assert rc == 0
    return table, ann, xc


@pytest.fixture(scope='module')
def reference():
    """The quadruples of every year count and their restatement, with AET and without, computed once."""
    out = {}
    for ny in cases.YEARS:
        p, pet, q, aet = cases.rows(ny)
        out[ny] = ((p, pet, q, aet), {True: wnp.water_balance(p, pet, q, aet, 0, ny, cases.MAX_LAG, cases.OMEGA0),
                                      False: wnp.water_balance(p, pet, q, None, 0, ny, cases.MAX_LAG, cases.OMEGA0)})
    return out


# ------------------------------------------------------------------ the rows and the restatement
def test_the_rows_cover_what_they_should(reference):
    assert cases.YEARS == (1, 2, 3, 5, 21, 22, 33, 64, 65, 257, 341) and len(cases.KINDS) == 15 and wnp.COLUMNS[11] == 'omega'
    k = {name: i for i, name in enumerate(cases.KINDS)}
    col = {name: i for i, name in enumerate(wnp.COLUMNS)}
    for ny, ((p, pet, q, aet), ref) in reference.items():
        table, annual, xcorr = ref[True]
        bare = ref[False][0]
        assert p.shape == (15, 12 * ny) and annual.shape == (15, 4, ny) and xcorr.shape == (15, cases.MAX_LAG + 1)
        assert table[k['humid'], col['aridity']] < 1 < table[k['arid'], col['aridity']] and table[k['equal'], col['aridity']] == 1.0
        assert table[k['q_zero'], col['q_mean']] == 0 and table[k['q_zero'], col['runoff_ratio']] == 0
        assert np.isnan(table[k['q_zero'], [11, 13, 14, 15, 16, 17, 19, 20]]).all()
        assert table[k['q_over_p'], col['runoff_ratio']] > 1 and np.isnan(table[k['q_over_p'], col['omega']])
        assert np.isnan(table[k['p_const'], [13, 15, 16, 17]]).all()                       # no qualifying year, det = 0
        assert table[k['collinear'], col['aridity']] == 2.0 and np.isnan(table[k['collinear'], [15, 16]]).all()
        assert same_bits(table[k['collinear'], 13], table[k['collinear'], 14])
        assert table[k['all_nan'], 0] == 0 and table[k['all_nan'], 1] == 0 and np.isnan(table[k['all_nan'], 2:]).all()
        assert np.isnan(annual[k['all_nan']]).all() and np.isnan(xcorr[k['all_nan']]).all()
        assert table[k['year_nan'], 0] == ny - 1 and table[k['year_nan'], 1] == 12 * (ny - 1)
        assert np.isnan(annual[k['year_nan'], :, ny // 2]).all()
        assert (np.signbit(p[k['signed_zeros']]) & (p[k['signed_zeros']] == 0)).any()
        assert np.isinf(q[k['scattered']]).any() or ny < 3
        # without AET: its columns are NaN, its plane too, and the gaps of AET alone are months again
        assert np.isnan(bare[:, [4, 8, 9, 10]]).all() and np.isnan(ref[False][1][:, 2]).all()
        assert bare[k['no_aet'], 1] == 12 * ny and (table[k['no_aet'], 1] < 12 * ny or ny < 3)
        others = [c for c in range(wnp.NCOL) if c not in (4, 8, 9, 10)]
        keep = [i for i in range(15) if i != k['no_aet']]
        assert same_bits(bare[keep][:, others], table[keep][:, others])
        if ny == 1:
            assert np.isnan(table[:, [13, 14, 15, 16, 17]]).all()                          # one year: dP = 0, no fit
        if ny == 2:
            assert np.isnan(table[:, [15, 16]]).all() and not np.isnan(table[k['humid'], 13])
        if ny >= 5:
            assert table[k['lagged'], col['lag_peak']] == 3 and table[k['lagged'], col['r_peak']] > 0.9
            assert not np.isnan(table[k['humid']]).any() and not np.isnan(table[k['arid']]).any()
            assert 1 < table[k['humid'], col['omega']] < 129 and abs(table[k['humid'], col['closure']]) < 0.2
            e = np.sort((annual[k['ties'], 3] - table[k['ties'], 5]) / (annual[k['ties'], 0] - table[k['ties'], 2]))
            assert (np.diff(e) == 0).any()                                                  # ties among the e_y


def test_median_correlation_and_least_squares_against_numpy(reference):
    """On the well-conditioned rows (humid, arid; 5 years and more) the elasticities are np.median of the annual ratios bit for
    bit where the count is odd and within 2 ulp where it is even (numpy halves the sum of the two middle values, the linear rule
    adds half their difference), r_pq is np.corrcoef's and the least-squares pair is np.linalg.lstsq's of z on (x1, x2), within
    1e-9: those routines sum pairwise and factorise."""
    for ny, ((p, pet, q, aet), ref) in reference.items():
        table, annual, xcorr = ref[True]
        for i in (0, 1):
            if ny < 5:
                continue
            A = annual[i]
            pbar, petbar, qbar = table[i, 2], table[i, 3], table[i, 5]
            dp, de, dq = A[0] - pbar, A[1] - petbar, A[3] - qbar
            for c, d, bar in ((13, dp, pbar), (14, de, petbar)):
                m = np.median((dq / d) * (bar / qbar))
                assert same_bits(table[i, c], m) if ny % 2 else abs(table[i, c] - m) <= 2 * EPS * abs(m), (ny, i, c)
            assert abs(table[i, 17] - np.corrcoef(A[0], A[3])[0, 1]) <= 1e-12
            X = np.stack([dp / pbar, de / petbar], axis=1)
            b = np.linalg.lstsq(X, dq / qbar, rcond=None)[0]
            assert np.allclose(table[i, 15:17], b, rtol=1e-9, atol=1e-12), (ny, i, table[i, 15:17], b)
            # the cross-correlation at lag 0 is np.corrcoef of the months
            assert abs(xcorr[i, 0] - np.corrcoef(p[i], q[i])[0, 1]) <= 1e-12
            assert table[i, 20] == xcorr[i].max() and table[i, 19] == np.argmax(xcorr[i])


def test_fu_and_its_root(probe):
    """Fu's curve in the definition's form against the textbook form at 40 digits, where the textbook form is harmless to
    evaluate, and the root put back into the curve; the host build and the restatement."""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(5)
    phi = np.ascontiguousarray(np.exp(rng.uniform(np.log(0.05), np.log(50.0), 300)))
    omega = np.exp(rng.uniform(np.log(1.05), np.log(20.0), 300))
    eps = np.ascontiguousarray([float(1 + mp.mpf(f) - (1 + mp.mpf(f) ** w) ** (1 / mp.mpf(w))) for f, w in zip(phi, omega)])
    got = np.full(300, -777.0)
    probe.wp_omega(300, phi.ctypes.data_as(P), eps.ctypes.data_as(P), got.ctypes.data_as(P))
    mine = np.array([wnp.omega_of(f, e) for f, e in zip(phi, eps)])
    for name, w in (('host build', got), ('restatement', mine)):
        back = np.array([float(1 + mp.mpf(f) - (1 + mp.mpf(f) ** mp.mpf(v)) ** (1 / mp.mpf(v))) for f, v in zip(phi, w)])
        # the curve at the root is eps again to a few ulp of the quantities of size <= 1 it is made of
        # (eps rounds to min(1, phi) itself for a few of the largest omega: no root there, and NaN from both)
        assert np.array_equal(np.isnan(w), ~(eps < np.minimum(1.0, phi))) and np.isnan(w).sum() < 30, name
        assert np.nanmax(np.abs(back - eps)) <= 16 * EPS, (name, np.nanmax(np.abs(back - eps)))
    one = np.full(1, -777.0)
    for f in (0.3, 1.0, 7.0):
        f_arr = np.array([f])
        probe.wp_fu(1, f_arr.ctypes.data_as(P), 2.6, one.ctypes.data_as(P))
        want = float(1 + mp.mpf(f) - (1 + mp.mpf(f) ** mp.mpf(2.6)) ** (1 / mp.mpf(2.6)))
        assert abs(one[0] - want) <= 4 * EPS and abs(wnp.fu(f, 2.6) - want) <= 4 * EPS
    # outside the curve's reach, and the two literals
    for f, e in ((0.5, 0.5), (0.5, 0.6), (2.0, 1.0), (2.0, 0.0), (2.0, -0.1), (np.nan, 0.3), (0.5, np.nan), (0.0, 0.0), (np.inf, 0.5)):
        f_arr, e_arr = np.array([f]), np.array([e])
        probe.wp_omega(1, f_arr.ctypes.data_as(P), e_arr.ctypes.data_as(P), one.ctypes.data_as(P))
        assert np.isnan(one[0]) and np.isnan(wnp.omega_of(f, e)), (f, e)
    assert wnp.S_LO == float(mp.log(mp.mpf(2) ** -20)) and wnp.S_HI == float(mp.log(mp.mpf(2) ** 7))


def tolerances(quad, with_aet, g, max_lag):
    """The bound on |value - 40-digit value| per column of one row, and that of xcorr: first-order error propagation.
    X = the largest magnitude among the included months, E = (12 nyear + 16) 2^-53 the rounding of a sum of that many terms.
    An annual total and a mean vbar err by d = 12 E X; a deviation dv_y by 2 d.  A quotient N / D errs by
    (dN + |N / D| dD) / |D|: runoff_ratio, aridity, evaporative (d (1 + |ratio|) / |pbar|), closure with residual's 3 d.
    e_y = (dQ_y / dP_y) (pbar / qbar) errs by (2 d (1 + |dQ_y / dP_y|) / |dP_y|) |pbar / qbar| + |e_y| d (1 / |pbar| + 1 / |qbar|), and
    a median moves by no more than the largest move of a value.  x = dv / vbar errs by dx = 2 d (1 + max|x|) / min|vbar|; each of
    the five sums of n products of them by dS = n (2 xm dx + E xm^2), xm = max|x|; det and both numerators (two products of sums
    <= n xm^2) by 4 n xm^2 dS: b errs by 4 n xm^2 dS (1 + |b|) / det.  r_pq is N / sqrt(Spp Sqq) with deviations of 2 d:
    4 n (12 X)^2 E (1 + |r|) / sqrt(Spp Sqq), and c_k and r_peak likewise over the months: 4 n X^2 E (1 + |c|) / sqrt(SPP SQQ).
    Every bound times 8 for the second-order terms and the roundings of the last operations.  dry_fraction is one division of
    two whole numbers: half an ulp of a quotient <= 1.  (|c| <= 1 stands for the c_k.)"""
    arrays = [np.asarray(a, dtype=np.float64) for a in quad[:3]] + ([np.asarray(quad[3], dtype=np.float64)] if with_aet else [])
    inc = np.logical_and.reduce([np.isfinite(a) for a in arrays])
    ncol = arrays[0].size
    ny = ncol // 12
    tol, tol_xcorr = np.zeros(wnp.NCOL), 0.0
    if not inc.any():
        return tol, tol_xcorr
    tol[18] = 2.0 ** -53                       # dry_fraction: one division of two whole numbers, a quotient <= 1
    X = max(float(np.abs(a[inc]).max()) for a in arrays)
    E = (ncol + 16) * 2.0 ** -53
    d = 12.0 * E * X
    with np.errstate(all='ignore'):
        pm, qm = arrays[0][inc], arrays[2][inc]
        SPP, SQQ = float(((pm - pm.mean()) ** 2).sum()), float(((qm - qm.mean()) ** 2).sum())
        tol_xcorr = tol[20] = 8.0 * 4.0 * inc.sum() * X * X * E * (1.0 + 1.0) / np.sqrt(SPP * SQQ) if SPP * SQQ > 0 else 0.0
        whole = inc.reshape(ny, 12).all(axis=1)
        n = float(whole.sum())
        if n == 0:
            return tol, tol_xcorr
        A = [a.reshape(ny, 12)[whole].sum(axis=1) for a in arrays[:3]]
        pbar, petbar, qbar = g[2], g[3], g[5]
        tol[2:6] = 8.0 * d
        for c in (6, 7, 8):
            tol[c] = 8.0 * d * (1.0 + abs(g[c])) / abs(pbar)
        tol[9] = 8.0 * 3.0 * d
        tol[10] = 8.0 * (3.0 * d + abs(g[10]) * d) / abs(pbar)
        dp, de, dq = A[0] - pbar, A[1] - petbar, A[2] - qbar
        for c, dv, bar in ((13, dp, pbar), (14, de, petbar)):
            sel = dv != 0.0
            if sel.any() and qbar > 0:
                ratio = dq[sel] / dv[sel]
                move = (2.0 * d * (1.0 + np.abs(ratio)) / np.abs(dv[sel])) * abs(bar / qbar) + np.abs(ratio * bar / qbar) * d * (1.0 / abs(bar) + 1.0 / abs(qbar))
                tol[c] = 8.0 * float(move.max())
        xs = np.concatenate([dp / pbar, de / petbar, dq / qbar])
        xm = float(np.abs(xs).max())
        dx = 2.0 * d * (1.0 + xm) / min(abs(pbar), abs(petbar), abs(qbar))
        dS = n * (2.0 * xm * dx + E * xm * xm)
        x1, x2 = dp / pbar, de / petbar
        det = float((x1 * x1).sum() * (x2 * x2).sum() - (x1 * x2).sum() ** 2)
        for c in (15, 16):
            tol[c] = 8.0 * 4.0 * n * xm * xm * dS * (1.0 + abs(g[c])) / det if det > 0 else 0.0
        spp, sqq = float((dp * dp).sum()), float((dq * dq).sum())
        tol[17] = 8.0 * 4.0 * n * (12.0 * X) ** 2 * E * (1.0 + abs(g[17])) / np.sqrt(spp * sqq) if spp * sqq > 0 else 0.0
    return tol, tol_xcorr


@pytest.mark.parametrize('years', cases.YEARS)
def test_restatement_and_host_build_against_40_digits(probe, reference, golden, years):
    g = golden('wbalance')
    quad, ref = reference[years]
    for with_aet in (True, False):
        key = '{}_{}'.format('' if with_aet else '_noaet', years)
        hi, lo, undef = g['table' + key], g['table_lo' + key], g['undef' + key]
        xhi, xlo = g['xcorr' + key], g['xcorr_lo' + key]
        host = host_balance(probe, quad[0], quad[1], quad[2], quad[3] if with_aet else None)
        for name, (table, annual, xcorr) in (('restatement', ref[with_aet]), ('host build', host)):
            tag = '{} {}{}'.format(name, years, '' if with_aet else ' without AET')
            assert np.array_equal(np.isnan(table) & ~undef, np.isnan(hi) & ~undef), tag
            for i in range(table.shape[0]):
                tol, tol_x = tolerances([a[i] for a in quad], with_aet, hi[i], cases.MAX_LAG)
                err = np.abs((table[i] - hi[i]) - lo[i])
                for c in BIT_COLUMNS:
                    if not np.isnan(hi[i, c]) and not undef[i, c]:
                        assert err[c] <= tol[c], (tag, cases.KINDS[i], wnp.COLUMNS[c], err[c], tol[c])
                if not undef[i, 20]:
                    e = np.abs((xcorr[i] - xhi[i]) - xlo[i])
                    assert np.array_equal(np.isnan(xcorr[i]), np.isnan(xhi[i])), (tag, cases.KINDS[i])
                    assert not (e > tol_x).any(), (tag, cases.KINDS[i], 'xcorr', np.nanmax(e), tol_x)
                # the annual totals are sums of 12: np.sum's pairwise order lies within 12 ulp of the largest month
                given = [a[i] for a in quad[:3]] + ([quad[3][i]] if with_aet else [])
                inc = np.logical_and.reduce([np.isfinite(a) for a in given]).reshape(years, 12).all(axis=1)
                for v, a in ((0, quad[0][i]), (1, quad[1][i]), (3, quad[2][i])) + (((2, quad[3][i]),) if with_aet else ()):
                    assert np.array_equal(np.isnan(annual[i, v]), ~inc), (tag, cases.KINDS[i], v)
                    yr = a.reshape(years, 12)[inc]
                    assert (np.abs(annual[i, v][inc] - yr.sum(axis=1)) <= 12 * EPS * np.abs(yr).max(axis=1, initial=0.0) * 12).all()
            bounded_columns(golden, table, years, with_aet, tag)


# ------------------------------------------------------------------ the host build of the header
@pytest.mark.parametrize('years', cases.YEARS)
def test_host_build_of_the_header_against_the_restatement(probe, reference, golden, years):
    quad, ref = reference[years]
    held(golden, host_balance(probe, *quad), ref[True], years, True, 'host build {}'.format(years))
    held(golden, host_balance(probe, quad[0], quad[1], quad[2], None), ref[False], years, False, 'host build {} without AET'.format(years))


def test_window_stride_lags_and_null_outputs(probe):
    quad = cases.rows(22)
    wide = [np.concatenate([a[:, -7:], a, a[:, :10]], axis=1) for a in quad]
    for start, nyear, max_lag, omega0 in ((0, 22, 6, 2.6), (7, 22, 0, 2.6), (17, 21, 12, 1.5), (9, 12, 3, 4.0)):
        got = host_balance(probe, *wide, start=start, nyear=nyear, max_lag=max_lag, omega0=omega0)
        ref = wnp.water_balance(*wide, start=start, nyear=nyear, max_lag=max_lag, omega0=omega0)
        assert got[2].shape == (15, max_lag + 1) and got[1].shape == (15, 4, nyear)
        assert same_bits(got[0][:, BIT_COLUMNS], ref[0][:, BIT_COLUMNS]) and same_bits(got[1], ref[1]) and same_bits(got[2], ref[2])
        assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0]))
        with np.errstate(invalid='ignore'):
            assert not (np.abs(got[0][:, 11:13] - ref[0][:, 11:13]) > 1e-12 * np.maximum(np.abs(ref[0][:, 11:13]), 1.0)).any()
    # a longer reach only adds lags
    a, b = host_balance(probe, *wide, start=7, nyear=22, max_lag=3), host_balance(probe, *wide, start=7, nyear=22, max_lag=12)
    assert same_bits(a[2], b[2][:, :4]) and same_bits(a[0][:, :19], b[0][:, :19])
    # NULL outputs are left alone
    full = host_balance(probe, *wide, start=7, nyear=22)
    for annual, xcorr in ((False, True), (True, False), (False, False)):
        got = host_balance(probe, *wide, start=7, nyear=22, annual=annual, xcorr=xcorr)
        assert got[0].tobytes() == full[0].tobytes()
        assert got[1].tobytes() == full[1].tobytes() if annual else (got[1] == -777.0).all()
        assert got[2].tobytes() == full[2].tobytes() if xcorr else (got[2] == -777.0).all()


def test_probe_refuses_what_the_entry_refuses(probe):
    x, t = np.ones((2, 130)), np.full((2, wnp.NCOL), -777.0)
    a, c = np.full((2, 4, 10), -777.0), np.full((2, 13), -777.0)

    def rc(stride=130, col0=0, nyear=10, max_lag=6, omega0=2.6, p=x, pet=x, q=x, table=t):
        ptr = [None if v is None else v.ctypes.data_as(P) for v in (p, pet, q)]
        return probe.wp_water_balance(2, stride, col0, nyear, max_lag, omega0, ptr[0], ptr[1], ptr[2], None,
                                      None if table is None else table.ctypes.data_as(P), a.ctypes.data_as(P), c.ctypes.data_as(P))
    for bad in (dict(p=None), dict(pet=None), dict(q=None), dict(table=None), dict(col0=-1), dict(col0=11), dict(nyear=0),
                dict(nyear=342, stride=5000), dict(max_lag=-1), dict(max_lag=13), dict(omega0=1.0), dict(omega0=0.5), dict(omega0=np.nan),
                dict(omega0=np.inf)):
        assert rc(**bad) == 1, bad
    assert (t == -777.0).all() and (a == -777.0).all() and (c == -777.0).all()
    assert rc() == 0 and (t[:, 0] == 10).all() and (t[:, 1] == 120).all() and (t[:, 2] == 12).all() and (c.ravel()[14:] == -777.0).all()      # ([2, 7] at the buffer's head)


def test_padded_sort_and_median_under_sanitizers(probe):
    """xh_wb_fill, xh_sig_sort and xh_wb_median in a stand-alone program of their own (tests/wbalance_probe/median_check.cpp,
    -fsanitize=address,undefined), started as a child process: every count 0 .. 341 of qualifying years among up to 341, with
    ties and signed zeros, teams of 1, 3 and 256 lanes, in buffers of exactly the sizes the kernel gives a workgroup, against
    std::sort."""
    out = subprocess.run([os.path.join(PROBE_DIR, 'median_check')], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and '1026 cases, 0 failed' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ------------------------------------------------------------------ the section
NM = 144


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('wbalance_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = synth.make_forcing(w, NM, seed=50)
    plain = synth.write_example(root, w, f, 1971, 1982, runoff_spinup=25, routing_spinup=6)
    ini = synth.write_example(root, w, f, 1971, 1982, runoff_spinup=25, routing_spinup=6, project='with_water_balance')
    synth.with_water_balance(ini, levels=('cell', 'basin'))
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
    assert '[WaterBalance]' in msg and all(k in msg for k in keys), msg
    return msg


LEVELS_LINE = r'levels = cell, basin'


def test_section_and_its_defaults(tree, tmp_path):
    root, w, f, plain, ini = tree
    from xanthos_amd import waterbalance
    c = ConfigReader(ini)
    assert c.CalculateWaterBalance == 1
    assert c.water_balance == {'levels': ['cell', 'basin'], 'start_year': 1971, 'end_year': 1982, 'year_start_month': 1, 'max_lag': 6,
                               'omega0': 2.6, 'annual': 0}
    c = ConfigReader(edited(ini, tmp_path, (LEVELS_LINE + r'\n', '')))
    assert c.water_balance['levels'] == ['cell']                                        # the default
    c = ConfigReader(edited(ini, tmp_path, (LEVELS_LINE, 'levels = Basin\nyear_start_month = 10\nstart_year = 1972\nmax_lag = 12\n'
                                            'omega0 = 1.8\nannual = 1')))
    # the year that starts in October 1981 is the last that ends inside 1982
    assert c.water_balance == {'levels': ['basin'], 'start_year': 1972, 'end_year': 1981, 'year_start_month': 10, 'max_lag': 12,
                               'omega0': 1.8, 'annual': 1}
    assert os.path.basename(waterbalance.output_stem(c, 'cell')) == 'water_balance_cell_with_water_balance'
    assert os.path.basename(waterbalance.output_stem(c, 'basin', 'xcorr')) == 'water_balance_basin_xcorr_with_water_balance'
    assert waterbalance.COLUMNS == wnp.COLUMNS and len(waterbalance.COLUMNS) == 21 and waterbalance.OMEGA0 == wnp.OMEGA0 == cases.OMEGA0
    assert waterbalance.csv_columns('cell')[2:6] == ('p_mean_mm', 'pet_mean_mm', 'aet_mean_mm', 'q_mean_mm')
    assert waterbalance.csv_columns('basin')[2:6] == ('p_mean_km3', 'pet_mean_km3', 'aet_mean_km3', 'q_mean_km3')
    assert waterbalance.csv_columns('basin')[:2] + waterbalance.csv_columns('basin')[6:] == wnp.COLUMNS[:2] + wnp.COLUMNS[6:]


def test_an_ini_without_the_flag_parses_as_before(tree):
    root, w, f, plain, ini = tree
    base = vars(ConfigReader(plain))
    assert base['CalculateWaterBalance'] == 0 and base['water_balance'] is None and 'WaterBalance' not in open(plain).read()
    with_flag = vars(ConfigReader(ini))
    differ = sorted(k for k in base if k not in ('CalculateWaterBalance', 'water_balance') and repr(base[k]) != repr(with_flag[k]))
    assert all('with_water_balance' in repr(with_flag[k]) for k in differ), differ       # only the project's name and its folders


def test_with_water_balance_writes_the_section(tree, tmp_path):
    root, w, f, plain, ini = tree
    path = str(tmp_path / 'enabled.ini')
    open(path, 'w').write(open(plain).read())
    assert synth.with_water_balance(path, levels=('basin',), year_start_month=4, max_lag=3, start_year=1973) == path
    text = open(path).read()
    assert 'CalculateWaterBalance = 1' in text.split('[PET]')[0] and text.rstrip().endswith('start_year = 1973')
    assert '[WaterBalance]\nlevels = basin\nyear_start_month = 4\nmax_lag = 3' in text
    c = ConfigReader(path)
    assert c.water_balance['max_lag'] == 3 and (c.water_balance['start_year'], c.water_balance['end_year']) == (1973, 1981)


def test_refusals_name_their_key(tree, tmp_path):
    root, w, f, plain, ini = tree
    refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell, region')), 'levels', 'region')
    refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell, cell')), 'levels')
    refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nmin_years = 10')), 'min_years', 'not a key')
    # a run without a runoff module
    no_runoff = ((r'(?s)\[Runoff\].*?\n\[Routing\]', '[Routing]'), (r'(?s)\[Routing\].*?\n\[WaterBalance\]', '[WaterBalance]'))
    refused(edited(ini, tmp_path, *no_runoff), 'runoff_module')
    # a run without a PET module: PET from a file
    pet_file = os.path.join(root, 'pet.npy')
    np.save(pet_file, np.ones((w.ncell, NM)))
    refused(edited(ini, tmp_path, (r'(?s)\[PET\].*?\n\[Runoff\]', '[PET]\npet_module = none\npet_file = {}\n\n[Runoff]'.format(pet_file))),
            'pet_module')
    # the window
    refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nstart_year = 1970')), 'start_year', '1970')
    refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nend_year = 1983')), 'end_year', '1983')
    refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nstart_year = soon')), 'start_year', 'soon')
    refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nstart_year = 1975\nend_year = 1974')), 'end_year', '1974', '1975')
    # fewer than 2 years
    refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nstart_year = 1975\nend_year = 1975')), 'end_year', '1975', 'at least 2')
    # an incomplete last year
    msg = refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nyear_start_month = 10\nend_year = 1982')), 'end_year', '1982', 'month 10')
    assert '1981' in msg
    for bad in ('0', '13', 'october'):
        refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nyear_start_month = ' + bad)), 'year_start_month', bad)
    for bad in ('-1', '13', 'long', '2.5'):
        refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nmax_lag = ' + bad)), 'max_lag', bad)
    for bad in ('1', '0.5', '-2', 'nan', 'inf', 'steep'):
        refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nomega0 = ' + bad)), 'omega0', bad)
    for bad in ('2', 'yes'):
        refused(edited(ini, tmp_path, (LEVELS_LINE, 'levels = cell\nannual = ' + bad)), 'annual', bad)
    refused(edited(ini, tmp_path, (r'OutputInYear = 0', 'OutputInYear = 1')), 'OutputInYear')
    # the flag and the section
    with pytest.raises(ValidationException, match='CalculateWaterBalance'):
        ConfigReader(edited(ini, tmp_path, (r'CalculateWaterBalance = 1', 'CalculateWaterBalance = yes')))
    with pytest.raises(ValidationException, match=r'CalculateWaterBalance = 1 but the config file has no \[WaterBalance\] section'):
        ConfigReader(edited(ini, tmp_path, (r'(?s)\n\[WaterBalance\].*$', '\n')))


def test_a_window_beyond_4096_months_is_refused(tree):
    root, w, f, plain, ini = tree
    c = ConfigReader(ini)
    c.StartYear, c.EndYear = 1700, 2041
    with pytest.raises(ValidationException) as exc:
        c.configure_water_balance({'levels': 'cell'})
    assert '[WaterBalance] end_year' in str(exc.value) and '4104 months' in str(exc.value) and '4096' in str(exc.value)
    c.configure_water_balance({'levels': 'cell', 'year_start_month': '10'})          # 341 years
    assert c.water_balance['end_year'] == 2040


def test_calibration_ensembles_and_sharded_precipitation_are_refused(tree, tmp_path):
    root, w, f, plain, ini = tree
    c = ConfigReader(ini)
    c.calibrate = 1
    with pytest.raises(ValidationException, match=r'\[WaterBalance\] and Calibrate = 1'):
        c.configure_water_balance({'levels': 'cell'})
    c.calibrate = 0
    c.ensemble = {'members': 'members.csv'}
    with pytest.raises(ValidationException, match=r'\[WaterBalance\] and an \[Ensemble\] section'):
        c.configure_water_balance({'levels': 'cell'})
    with_ens = edited(ini, tmp_path, (r'(?s)$', '\n[Ensemble]\nmembers = members.csv\n'), name='ens.ini')
    try:
        ConfigReader(with_ens)
    except ValidationException as exc:          # whichever section speaks first, the run does not start
        assert '[WaterBalance]' in str(exc) or '[Ensemble]' in str(exc)
    else:
        raise AssertionError('an ini with [WaterBalance] and [Ensemble] was accepted')
    from xanthos_amd import ensemble
    with pytest.raises(ValidationException) as exc:
        ensemble.validate(ConfigReader(ini), [('a', {})])
    assert 'CalculateWaterBalance' in str(exc.value) and '[Ensemble]' in str(exc.value)
    # a sharded run: every rank's pipeline holds its own rows of the precipitation only
    from types import SimpleNamespace
    from xanthos_amd.components import Components
    comp = Components.__new__(Components)
    comp.s = SimpleNamespace(ncell=w.ncell, nmonths=NM)
    comp.pipe = SimpleNamespace(forcing={'precip': SimpleNamespace(shape=(w.ncell // 2, NM))})
    with pytest.raises(ValidationException) as exc:
        comp._precipitation('precip', 'WaterBalance')
    assert '[WaterBalance] levels' in str(exc.value) and 'several GPUs' in str(exc.value)


# ------------------------------------------------------------------ the C-ABI entry
def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    assert re.search(r'\bint xh_water_balance\(xh_ctx \*ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t max_lag, '
                     r'double omega0,\s+const double \*d_p, const double \*d_pet, const double \*d_q, const double \*d_aet, double \*d_table,\s+'
                     r'double \*d_annual, double \*d_xcorr\);', header)
    assert re.search(r'#define XH_WB_NCOL 21\b', header) and re.search(r'#define XH_WB_MAX_LAG 12\b', header)
    assert 'xh_water_balance replaces NO function of the reference' in header and 'timer "water_balance"' in header
    assert len(_hip.SIGNATURES['xh_water_balance'][1]) == 14
    assert hasattr(_hip.lib(), 'xh_water_balance') and _hip.lib().xh_abi_version() == _hip.ABI_VERSION == 7
    assert hasattr(_hip.Context, 'water_balance')
    dev = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'xh_wbalance_dev.h')).read()
    assert re.search(r'#define XH_WB_NCOL 21\b', dev) and re.search(r'#define XH_WB_BISECT 60\b', dev) and '#include "xh_signatures_dev.h"' in dev
    assert re.search(r'#define XH_WB_S_LO {!r}\b'.format(wnp.S_LO), dev) and re.search(r'#define XH_WB_S_HI {!r}\b'.format(wnp.S_HI), dev)
    hip = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'xh_wbalance.hip')).read()
    assert '"water_balance"' in hip and 'atomic' not in hip.replace('No atomics', '')
    make = open(os.path.join(ROOT, 'xanthos_amd', 'csrc', 'Makefile')).read()
    assert 'xh_wbalance.hip' in make and 'xh_wbalance.o: xh_wbalance.hip $(HDRS) xh_wbalance_dev.h xh_signatures_dev.h' in make
