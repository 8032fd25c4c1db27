"""xh_signatures on the device: every kind of row of tests/signatures_cases.py at every year count against the host
build of the same header (tests/signatures_probe), determinism, windows, numbers of probabilities, NULL outputs, the argument
errors, signature_rows on host and device arrays, and run_model with CalculateSignatures = 1.

Every column but fdc_slope and centroid must be the host build's bits, and so must the duration curve and the calendar means;
those two come through the device's log and atan2 and are held to the bounds of tests/test_signatures_host.py -- 4 x the
distance measured for the restatement from 40-digit values, per quantity, against those 40-digit values, on every row.  NaN
masks are identical.  64 rows per call: the 15 kinds over and over, one workgroup each."""
import os
import re

import numpy as np
import pytest

import signatures_cases as cases
import signatures_np as snp
from test_signatures_host import BIT_COLUMNS, PROBS, bounded_columns, host_signatures, probe, same_bits  # noqa: F401  (probe: the fixture)

pytestmark = pytest.mark.gpu
NROWS = 64
FILL = -7.0


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def device_signatures(ctx, rows, start=0, nyear=None, cal0=cases.CAL0, probs=PROBS, fdc=True, regime=True, fill=FILL):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    nyear = (rows.shape[1] - start) // 12 if nyear is None else nyear
    d_x = ctx.upload(rows)
    d_t = ctx.upload(np.full((rows.shape[0], snp.NCOL), fill))
    d_f, d_m = ctx.upload(np.full((rows.shape[0], max(len(probs), 1)), fill)), ctx.upload(np.full((rows.shape[0], 12), fill))
    ctx.signatures(rows.shape[0], rows.shape[1], start, nyear, cal0, probs, d_x, d_t, d_f if fdc else None, d_m if regime else None)
    out = d_t.download(), d_f.download().ravel()[:rows.shape[0] * len(probs)].reshape(rows.shape[0], len(probs)), d_m.download()
    tail = d_f.download().ravel()[rows.shape[0] * len(probs):]
    assert (tail == fill).all()                      # nothing is written past [nrows, nP]
    for a in (d_x, d_t, d_f, d_m):
        a.free()
    return out


def tiled(years):
    """64 rows: the 15 kinds over and over; row i is kind i mod 15."""
    return cases.rows(years)[np.arange(NROWS) % len(cases.KINDS)]


def same(got, ref, tag):
    assert same_bits(got[0][:, BIT_COLUMNS], ref[0][:, BIT_COLUMNS]), tag
    assert same_bits(got[1], ref[1]) and same_bits(got[2], ref[2]), tag
    assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0])), tag


@pytest.mark.parametrize('years', cases.YEARS)
def test_every_kind_of_row_at_every_year_count(ctx, probe, golden, years):  # noqa: F811
    rows = tiled(years)
    got = device_signatures(ctx, rows)
    same(got, host_signatures(probe, rows), 'device {}'.format(years))
    for first in range(0, NROWS - len(cases.KINDS) + 1, len(cases.KINDS)):                 # every copy of the 15 rows, none left out
        bounded_columns(golden, got[0][first:first + len(cases.KINDS)], years, 'device {} rows {}..'.format(years, first))
    assert got[0][-1].tobytes() == got[0][NROWS - 1 - len(cases.KINDS)].tobytes()          # (the last, incomplete copy)
    # two calls give identical bytes
    again = device_signatures(ctx, rows, fill=3.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_windows_strides_and_numbers_of_probabilities(ctx, probe):  # noqa: F811
    wide = tiled(22)
    wide = np.concatenate([wide[:, -7:], wide, wide[:, :10]], axis=1)
    sixteen = np.linspace(0.03, 0.97, 16)
    for start, nyear, cal0, probs in ((0, 22, 0, PROBS), (7, 22, 3, sixteen), (17, 21, 11, np.array([])), (9, 12, 6, np.array([0.5]))):
        got = device_signatures(ctx, wide, start, nyear, cal0, probs)
        assert got[1].shape == (NROWS, len(probs))
        same(got, host_signatures(probe, wide, start, nyear, cal0, probs), 'window {} {}'.format(start, nyear))
        slope, centroid = got[0][:, 8], got[0][:, 13]
        ref = snp.signatures(wide, start, nyear, cal0, probs)[0]
        with np.errstate(invalid='ignore'):                                           # (no 40-digit values of these windows: that
            assert not (np.abs(slope - ref[:, 8]) > 1e-12 * np.maximum(np.abs(ref[:, 8]), 1.0)).any()   # the columns are filled at all)
            d = np.abs(centroid - ref[:, 13])
            assert not (np.minimum(d, 12.0 - d) * ref[:, 14] > 1e-12).any()


def test_null_outputs_are_left_alone(ctx):
    rows = tiled(43)
    full = device_signatures(ctx, rows)
    for fdc, regime in ((False, True), (True, False), (False, False)):
        got = device_signatures(ctx, rows, fdc=fdc, regime=regime)
        assert got[0].tobytes() == full[0].tobytes()
        assert got[1].tobytes() == full[1].tobytes() if fdc else (got[1] == FILL).all()
        assert got[2].tobytes() == full[2].tobytes() if regime else (got[2] == FILL).all()


def test_argument_errors_launch_nothing(ctx):
    from xanthos_amd import _hip
    d_x, d_t = ctx.upload(np.ones((2, 5000))), ctx.upload(np.full((2, snp.NCOL), FILL))
    d_f, d_m = ctx.upload(np.full((2, 16), FILL)), ctx.upload(np.full((2, 12), FILL))
    lib = _hip.lib()
    p = np.array([0.5, 0.9])

    def refused(pattern, **bad):
        arg = dict(stride=130, col0=0, nyear=10, cal0=0, nP=2, p=p, x=d_x.ptr, table=d_t.ptr)
        arg.update(bad)
        rc = lib.xh_signatures(ctx.handle, 2, arg['stride'], arg['col0'], arg['nyear'], arg['cal0'], arg['nP'],
                               None if arg['p'] is None else arg['p'].ctypes.data, arg['x'], arg['table'], d_f.ptr, d_m.ptr)
        assert rc == 1, bad
        with pytest.raises(_hip.HipError) as exc:
            ctx._check(rc)
        assert 'error 1' in str(exc.value) and re.search(pattern, str(exc.value)), str(exc.value)
    refused('NULL array', x=None)
    refused('NULL array', table=None)
    refused(r'NULL probabilities with nP = 2', p=None)
    refused(r'column -1', col0=-1)
    refused(r'column 11, 10 years = 120 columns', col0=11)
    refused(r'nyear \(0\)', nyear=0)
    refused(r'nyear \(342\)', nyear=342, stride=5000)
    refused(r'cal0 \(-1\)', cal0=-1)
    refused(r'cal0 \(12\)', cal0=12)
    refused(r'nP \(-1\)', nP=-1)
    refused(r'nP \(17\)', nP=17)
    refused(r'probability 1 \(1\)', p=np.array([0.5, 1.0]))
    refused(r'probability 0 \(0\)', p=np.array([0.0, 0.5]))
    refused(r'probability 0 \(nan\)', p=np.array([np.nan, 0.5]))
    ctx.sync()
    assert (d_t.download() == FILL).all() and (d_f.download() == FILL).all() and (d_m.download() == FILL).all()
    before = ctx.timing('signatures')[1]
    ctx.signatures(2, 5000, 908, 341, 0, p, d_x, d_t, d_f, d_m)               # the longest window there is, to the row's last column
    ctx.sync()
    assert ctx.timing('signatures')[1] == before + 1                          # the timer's name
    out = d_t.download()
    assert (out[:, 0] == 4092).all() and (out[:, [2, 5, 16]] == [1.0, 1.0, 12.0]).all() and (out[:, [3, 7, 12, 17]] == 0.0).all()
    curve = d_f.download().ravel()                                            # [2, nP = 2] at the head of the [2, 16] buffer
    assert (curve[:4] == 1.0).all() and (curve[4:] == FILL).all() and (d_m.download() == 1.0).all()
    for a in (d_x, d_t, d_f, d_m):
        a.free()


def test_signature_rows_on_host_and_device_arrays(ctx, probe):  # noqa: F811
    from xanthos_amd import _hip, signatures
    rows = tiled(21)[:40]
    host = signatures.signature_rows(ctx, rows, cal0=cases.CAL0)
    d_rows = ctx.upload(rows)
    dev = signatures.signature_rows(ctx, d_rows, cal0=cases.CAL0)
    assert all(isinstance(a, _hip.DeviceArray) for a in host) and [tuple(a.shape) for a in host] == [(40, 18), (40, 9), (40, 12)]
    a, b = [x.download() for x in host], [x.download() for x in dev]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    same(a, host_signatures(probe, rows), 'signature_rows')
    win = signatures.signature_rows(ctx, d_rows, start=24, nyear=10, cal0=5, exceedance=(95, 0.5))
    same([x.download() for x in win], host_signatures(probe, rows, 24, 10, 5, np.array([0.05, 0.995])), 'signature_rows window')
    # a gauge record with gaps is a host array like any other
    record = np.where(np.arange(252) % 7 == 0, np.nan, rows[:1])
    gauge = signatures.signature_rows(ctx, record)
    assert gauge[0].download()[0, 0] == 216 and same_bits(gauge[1].download(), snp.signatures(record)[1])
    with pytest.raises(ValueError, match='nrows, ncols'):
        signatures.signature_rows(ctx, rows[0])
    with pytest.raises(_hip.HipError, match='probability 0'):
        signatures.signature_rows(ctx, d_rows, exceedance=(100,))
    for x in host + dev + win + gauge + (d_rows,):
        x.free()


# ------------------------------------------------------------------ run_model
PROJECT = 'pm_abcd_mrtm_synth'
YEARS = (1971, 1982)
NPY = 4
VARS = {'q': 'q_mmpermonth', 'avgchflow': 'avgchflow_m3persec'}
PERCENTS = (5, 33, 50, 66, 95, 99.5)        # (33 and 66: Q(0.67) and Q(0.34), what fdc_slope is made of)


def files_of(folder, skip=('logfile.log',)):
    out = {}
    for base, _, names in os.walk(folder):
        for f in names:
            if f not in skip:
                out[os.path.relpath(os.path.join(base, f), folder)] = os.path.join(base, f)
    return out


def test_run_model_writes_the_signatures_and_nothing_else_changes(tmp_path):
    import filecmp
    import mpmath as mp
    from xanthos_amd import run_model, synth
    mp.mp.dps = 40
    w = synth.make_world(nrow=48, ncol=96, ncell=2000, n_basins=8, seed=21)
    nm = 12 * (YEARS[1] - YEARS[0] + 1)
    forcing = synth.make_forcing(w, nm, seed=100)

    def example(root, on):
        ini = synth.write_example(str(root), w, forcing, YEARS[0], YEARS[1], runoff_spinup=25, routing_spinup=6,
                                  output_vars=('q', 'avgchflow', 'soilmoisture'), output_format=NPY)
        if on:
            synth.with_signatures(ini, signature_vars=('q', 'avgchflow'), exceedance=PERCENTS, year_start_month=10)
        return ini
    run_model(example(tmp_path / 'plain', False))
    c = run_model(example(tmp_path / 'signatures', True))
    out_plain, out = [os.path.join(str(tmp_path), d, 'output', PROJECT) for d in ('plain', 'signatures')]
    fa, fb = files_of(out_plain), {k: v for k, v in files_of(out).items() if not k.startswith('signatures_')}
    assert sorted(fa) == sorted(fb) and fa
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), rel                     # every other file byte for byte
    names = ['signatures_{}{}_{}.{}'.format(v, what, PROJECT, e) for v in VARS
             for what, e in (('', 'npy'), ('', 'csv'), ('_fdc', 'npy'), ('_fdc', 'csv'), ('_regime', 'npy'))]
    assert sorted(k for k in files_of(out) if k.startswith('signatures_')) == sorted(names)
    # years from October: 1971/72 .. 1981/82, the last one ending with the run's last month
    m0, nyear = 9, 11
    assert sorted(c.signatures) == sorted(VARS)
    probs = snp.probabilities(PERCENTS)
    for var, name in VARS.items():
        x = np.load(os.path.join(out, '{}_{}.npy'.format(name, PROJECT)))           # the run's own output array
        assert x.shape == (w.ncell, nm)
        want = snp.signatures(x, m0, nyear, 9, probs)
        stem = os.path.join(out, 'signatures_' + var)
        got = (np.load('{}_{}.npy'.format(stem, PROJECT)), np.load('{}_fdc_{}.npy'.format(stem, PROJECT)),
               np.load('{}_regime_{}.npy'.format(stem, PROJECT)))
        assert got[0].shape == (w.ncell, 18) and got[1].shape == (w.ncell, 6) and got[2].shape == (w.ncell, 12)
        same(got, want, 'run_model ' + var)
        # fdc_slope and centroid against 40-digit values formed from what they are made of, which the lines above hold to the
        # restatement's bits: Q(0.67) and Q(0.34) are the curve's columns 33 and 66, C and S come from the calendar means.
        # Each log is within an ulp of its value, their difference and the quotient within half an ulp each: 4 ulp of the
        # largest magnitude involved, over 0.33.  The centroid's measure and bound are those of the case rows (4 x 2^-49).
        assert probs[1] == 0.67 and probs[3] == 0.34
        for i in range(w.ncell):
            q67, q34 = got[1][i, 1], got[1][i, 3]
            assert np.isnan(got[0][i, 8]) == (not q34 > 0.0)
            if q34 > 0.0:
                l67, l34 = mp.log(mp.mpf(float(q67))), mp.log(mp.mpf(float(q34)))
                ref = (l67 - l34) / mp.mpf(0.33)
                tol = 4.0 * 2.0 ** -52 * max(abs(float(l67)), abs(float(l34)), abs(float(ref)), 1.0) / 0.33
                assert abs(float(mp.mpf(float(got[0][i, 8])) - ref)) <= tol, (var, i, got[0][i, 8], float(ref), tol)
            assert np.isnan(got[0][i, 13]) == bool(np.isnan(got[2][i]).any())
            if not np.isnan(got[0][i, 13]):
                xm = [mp.mpf(float(v)) for v in got[2][i]]
                C = mp.fsum(xm[m] * mp.mpf(float(snp.COS[m])) for m in range(12))
                S = mp.fsum(xm[m] * mp.mpf(float(snp.SIN[m])) for m in range(12))
                ref = mp.atan2(S, C) * mp.mpf(snp.MONTHS_PER_RADIAN)
                ref = ref + 12 if ref < 0 else ref
                d = abs(mp.mpf(float(got[0][i, 13])) - ref)
                err = float(min(d, 12 - d) * mp.sqrt(C * C + S * S) / mp.fsum(xm)) if mp.fsum(xm) != 0 else 0.0
                assert err <= 4.0 * 2.0 ** -49, (var, i, got[0][i, 13], float(ref), err)
        res = c.signatures[var]
        assert all(res[k].tobytes() == a.tobytes() for k, a in zip(('table', 'fdc', 'regime'), got))
        # (a cell whose forcing has a NaN month has NaN results from there on: fewer months, or none)
        assert (got[0][:, 0] == np.isfinite(x[:, m0:m0 + 12 * nyear]).sum(axis=1)).all() and (got[0][:, 0] == 12 * nyear).sum() > w.ncell // 2
        assert (~np.isnan(got[0][:, 13])).sum() > w.ncell // 2
        for what, arr, header in (('', got[0], 'id,' + ','.join(snp.COLUMNS)), ('_fdc', got[1], 'id,Q5,Q33,Q50,Q66,Q95,Q99.5')):
            lines = open('{}{}_{}.csv'.format(stem, what, PROJECT)).read().splitlines()
            assert lines[0] == header and len(lines) == w.ncell + 1
            text = np.array([[float(v or 'nan') for v in ln.split(',')] for ln in lines[1:]])   # (NaN is the empty field)
            assert (text[:, 0] == np.arange(1, w.ncell + 1)).all()                 # ids from 1
            assert np.array_equal(text[:, 1:], arr, equal_nan=True)                # the csv parses back to the npy exactly
