"""xh_extremes on the device: the rows of tests/extremes_cases.py at every year count and both kinds against the
host build of the same header (tests/extremes_probe), determinism, windows, handed-in parameters, NULL outputs, the argument
errors, extremes_rows on host and device arrays, and run_model with CalculateExtremes = 1.

n, the annual series, l1, l2, t3 and t4 must be the host build's bits; k, alpha, xi, the return levels and T_y come through the
device's expm1, log1p, exp, log and tgamma and are held to the bounds of tests/test_extremes_host.py -- 4 x the error measured
for the restatement against 40-digit values on these very 300 rows, per quantity and row class.  NaN masks are identical.
300 rows per call: 75 workgroups of four wavefronts."""
import os
import re

import numpy as np
import pytest

import extremes_cases as cases
import extremes_np
from test_extremes_host import host_extremes, probe, within  # noqa: F401  (probe: the fixture)

pytestmark = pytest.mark.gpu
NROWS = 300
FILL = -7.0


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def device_extremes(ctx, rows, kind, T=cases.GOLDEN_T, min_years=cases.MIN_YEARS, start=0, nyear=None, parameters=None,
                    annual=True, T_year=True, fill=FILL):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    nyear = (rows.shape[1] - start) // 12 if nyear is None else nyear
    d_x = ctx.upload(rows)
    d_t = ctx.upload(np.full((rows.shape[0], 8 + len(T)), fill))
    d_a, d_ty = ctx.upload(np.full((rows.shape[0], nyear), fill)), ctx.upload(np.full((rows.shape[0], nyear), fill))
    d_p = None if parameters is None else ctx.upload(np.ascontiguousarray(np.asarray(parameters)[:, :8]))
    ctx.extremes(rows.shape[0], rows.shape[1], start, nyear, kind, min_years, T, d_x, d_t, d_a if annual else None,
                 d_ty if T_year else None, d_p)
    out = d_t.download(), d_a.download(), d_ty.download()
    for a in (d_x, d_t, d_a, d_ty, d_p):
        if a is not None:
            a.free()
    return out


def held(golden, got, ref, tag, **kw):
    assert cases.bits_equal(got[0], got[1], ref[0], ref[1]), tag
    within(golden, got, ref, tag, **kw)


@pytest.mark.parametrize('kind', extremes_np.KINDS)
@pytest.mark.parametrize('years', cases.YEARS)
def test_every_kind_of_row_at_every_year_count(ctx, probe, golden, years, kind):  # noqa: F811
    rows = cases.make_rows(years, NROWS)
    got = device_extremes(ctx, rows, kind)
    ref = host_extremes(probe, rows, kind)
    held(golden, got, ref, '{} {}'.format(years, kind))
    assert (~np.isnan(ref[0][:, 5])).sum() > NROWS // 3 and np.isnan(ref[0][:, 5]).sum() > NROWS // 10
    # two calls give identical bytes
    again = device_extremes(ctx, rows, kind, fill=3.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_windows_strides_and_numbers_of_periods(ctx, probe, golden):  # noqa: F811
    wide = cases.make_rows(30, NROWS)
    wide = np.concatenate([wide[:, -7:], wide, wide[:, :10]], axis=1)
    for start, nyear, T in ((0, 30, (2.0,)), (7, 30, (1.5, 2, 5, 10, 20, 50, 100, 500)), (17, 29, ()), (9, 12, (10.0, 3.0))):
        for kind in extremes_np.KINDS:
            got = device_extremes(ctx, wide, kind, T=T, start=start, nyear=nyear)
            assert got[0].shape == (NROWS, 8 + len(T))
            held(golden, got, host_extremes(probe, wide, kind, T=T, start=start, nyear=nyear), 'window {} {} {}'.format(start, nyear, kind))
    a = device_extremes(ctx, wide, 'max', start=7, nyear=12, min_years=13)
    assert np.isnan(a[0][:, 3:]).all() and np.isnan(a[2]).all() and not np.isnan(a[0][:, :3]).all()


def test_parameters_handed_in(ctx, probe, golden):  # noqa: F811
    hist, future = cases.make_rows(50, NROWS), cases.make_rows(10, NROWS, seed=7) * 1.2
    for kind in extremes_np.KINDS:
        table = device_extremes(ctx, hist, kind)[0]
        got = device_extremes(ctx, future, kind, T=(10.0, 100.0), parameters=table)
        assert got[0][:, :8].tobytes() == table[:, :8].tobytes()
        ref = host_extremes(probe, future, kind, T=(10.0, 100.0), parameters=table)
        assert got[1].tobytes() == ref[1].tobytes()
        within(golden, got, ref, 'parameters ' + kind, quantities=('level', 'T_year'))


def test_null_outputs_are_left_alone(ctx):
    rows = cases.make_rows(64, NROWS)
    full = device_extremes(ctx, rows, 'max')
    for annual, T_year in ((False, True), (True, False), (False, False)):
        got = device_extremes(ctx, rows, 'max', annual=annual, T_year=T_year)
        assert got[0].tobytes() == full[0].tobytes()
        assert got[1].tobytes() == full[1].tobytes() if annual else (got[1] == FILL).all()
        assert got[2].tobytes() == full[2].tobytes() if T_year else (got[2] == FILL).all()


def test_argument_errors_launch_nothing(ctx):
    from xanthos_amd import _hip
    d_x, d_t = ctx.upload(np.ones((2, 5000))), ctx.upload(np.full((2, 10), FILL))
    d_a, d_ty = ctx.upload(np.full((2, 341), FILL)), ctx.upload(np.full((2, 341), FILL))
    lib = _hip.lib()
    T = np.array([2.0, 10.0])

    def refused(pattern, **bad):
        arg = dict(stride=130, col0=0, nyear=10, kind=0, min_years=5, nT=2, T=T, x=d_x.ptr, table=d_t.ptr)
        arg.update(bad)
        rc = lib.xh_extremes(ctx.handle, 2, arg['stride'], arg['col0'], arg['nyear'], arg['kind'], arg['min_years'], arg['nT'],
                             None if arg['T'] is None else arg['T'].ctypes.data, arg['x'], None, arg['table'], d_a.ptr, d_ty.ptr)
        assert rc == 1, bad
        with pytest.raises(_hip.HipError) as exc:
            ctx._check(rc)
        assert 'error 1' in str(exc.value) and re.search(pattern, str(exc.value)), str(exc.value)
    refused('NULL', x=None)
    refused('NULL', table=None)
    refused('NULL return periods', T=None)
    refused(r'column -1', col0=-1)
    refused(r'column 11, 10 years = 120 columns', col0=11)
    refused(r'nyear \(0\)', nyear=0)
    refused(r'nyear \(342\)', nyear=342, stride=5000)
    refused(r'nT \(-1\)', nT=-1)
    refused(r'nT \(9\)', nT=9)
    refused(r'return period 1 \(1\)', T=np.array([2.0, 1.0]))
    refused(r'return period 0', T=np.array([np.nan, 3.0]))
    refused(r'kind \(2\)', kind=2)
    refused(r'kind \(-1\)', kind=-1)
    refused(r'min_years \(4\)', min_years=4)
    ctx.sync()
    assert (d_t.download() == FILL).all() and (d_a.download() == FILL).all() and (d_ty.download() == FILL).all()
    before = ctx.timing('extremes')[1]
    ctx.extremes(2, 5000, 908, 341, 'max', 5, T, d_x, d_t, d_a, d_ty)       # the longest window there is, to the row's last column
    ctx.sync()
    assert ctx.timing('extremes')[1] == before + 1                          # the timer's name
    out = d_t.download()
    assert (out[:, 0] == 341).all() and (out[:, 1] == 1.0).all() and (np.abs(out[:, 2]) < 1e-13).all() and np.isnan(out[:, 3:]).all()
    assert (d_a.download() == 1.0).all() and np.isnan(d_ty.download()).all()
    for a in (d_x, d_t, d_a, d_ty):
        a.free()


def test_extremes_rows_on_host_and_device_arrays(ctx, probe, golden):  # noqa: F811
    from xanthos_amd import _hip, extremes
    rows = cases.make_rows(50, 40)
    host = extremes.extremes_rows(ctx, rows, 'min', min_years=5)
    d_rows = ctx.upload(rows)
    dev = extremes.extremes_rows(ctx, d_rows, 'min', min_years=5)
    assert all(isinstance(a, _hip.DeviceArray) for a in host) and [tuple(a.shape) for a in host] == [(40, 14), (40, 50), (40, 50)]
    a, b = [x.download() for x in host], [x.download() for x in dev]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    held(golden, a, host_extremes(probe, rows, 'min', T=extremes.RETURN_PERIODS), 'extremes_rows')
    win = extremes.extremes_rows(ctx, d_rows, 'max', start=24, nyear=20, return_periods=(10.0,), parameters=host[0])
    w = [x.download() for x in win]
    held(golden, w, host_extremes(probe, rows, 'max', T=(10.0,), start=24, nyear=20, parameters=a[0]), 'extremes_rows window',
         quantities=('level', 'T_year'))
    with pytest.raises(ValueError, match='kind'):
        extremes.extremes_rows(ctx, d_rows, 'mean')
    with pytest.raises(ValueError, match='parameters'):
        extremes.extremes_rows(ctx, d_rows, 'max', parameters=np.zeros((39, 8)))
    with pytest.raises(_hip.HipError, match='min_years'):
        extremes.extremes_rows(ctx, d_rows, 'max', min_years=3)
    for x in host + dev + win + (d_rows,):
        x.free()


# ------------------------------------------------------------------ run_model
PROJECT = 'pm_abcd_mrtm_synth'
YEARS = (1971, 1982)
NPY = 4
PERIODS = (2.0, 10.0, 100.0)
VARS = {'q': 'q_mmpermonth', 'avgchflow': 'avgchflow_m3persec'}


def files_of(folder, skip=('logfile.log',)):
    out = {}
    for base, _, names in os.walk(folder):
        for f in names:
            if f not in skip:
                out[os.path.relpath(os.path.join(base, f), folder)] = os.path.join(base, f)
    return out


def test_run_model_writes_the_extremes_and_nothing_else_changes(tmp_path, golden):
    import filecmp
    from xanthos_amd import run_model, synth
    w = synth.make_world(nrow=48, ncol=96, ncell=2000, n_basins=8, seed=21)
    nm = 12 * (YEARS[1] - YEARS[0] + 1)
    forcing = synth.make_forcing(w, nm, seed=100)

    def example(root, **keys):
        ini = synth.write_example(str(root), w, forcing, YEARS[0], YEARS[1], runoff_spinup=25, routing_spinup=6,
                                  output_vars=('q', 'avgchflow', 'soilmoisture'), output_format=NPY)
        if keys:
            synth.enable_extremes(ini, extreme_vars=('q', 'avgchflow'), kinds=('max', 'min'), return_periods=PERIODS,
                                  year_start_month=10, **keys)
        return ini
    run_model(example(tmp_path / 'plain'))
    c = run_model(example(tmp_path / 'extremes', min_years=10))
    out_plain, out = [os.path.join(str(tmp_path), d, 'output', PROJECT) for d in ('plain', 'extremes')]
    fa, fb = files_of(out_plain), {k: v for k, v in files_of(out).items() if not k.startswith('extremes_')}
    assert sorted(fa) == sorted(fb) and fa
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), rel                     # every other file byte for byte
    names = ['extremes_{}_{}{}_{}.{}'.format(v, k, what, PROJECT, e) for v in VARS for k in ('max', 'min')
             for what, e in (('', 'npy'), ('', 'csv'), ('_annual', 'npy'), ('_return_period', 'npy'))]
    assert sorted(k for k in files_of(out) if k.startswith('extremes_')) == sorted(names)
    # hydrological years from October: 1971/72 .. 1981/82, the last one ending with the run's last month
    m0, nyear = 9, 11
    assert sorted(c.extremes) == sorted((v, k) for v in VARS for k in ('max', 'min'))

    def check(folder, results, parameters=None):
        for var, name in VARS.items():
            x = np.load(os.path.join(folder, '{}_{}.npy'.format(name, PROJECT)))           # the run's own output array
            assert x.shape == (w.ncell, nm)
            for kind in ('max', 'min'):
                par = None if parameters is None else parameters[(var, kind)]
                want = extremes_np.extremes_rows(x, kind, PERIODS, min_years=10, start=m0, nyear=nyear, parameters=par)
                stem = os.path.join(folder, 'extremes_{}_{}'.format(var, kind))
                got = (np.load('{}_{}.npy'.format(stem, PROJECT)), np.load('{}_annual_{}.npy'.format(stem, PROJECT)),
                       np.load('{}_return_period_{}.npy'.format(stem, PROJECT)))
                assert got[0].shape == (w.ncell, 11) and got[1].shape == got[2].shape == (w.ncell, nyear)
                assert cases.bits_equal(got[0], got[1], want[0], want[1])
                within(golden, got, want, 'run_model {} {}'.format(var, kind), classes='ordinary',
                       quantities=cases.QUANTITIES if parameters is None else ('level', 'T_year'))
                res = results[(var, kind)]
                assert all(res[k].tobytes() == a.tobytes() for k, a in zip(('table', 'annual', 'return_period'), got))
                # (a cell whose forcing has a NaN month has NaN results from there on: fewer years, or none)
                assert (got[0][:, 0] == (~np.isnan(got[1])).sum(axis=1)).all() and (got[0][:, 0] == nyear).sum() > w.ncell // 2
                assert (~np.isnan(got[0][:, 5])).sum() > w.ncell // 2
                lines = open('{}_{}.csv'.format(stem, PROJECT)).read().splitlines()
                assert lines[0] == 'id,n,l1,l2,t3,t4,k,alpha,xi,x_T2,x_T10,x_T100' and len(lines) == w.ncell + 1
                text = np.array([[float(v or 'nan') for v in ln.split(',')] for ln in lines[1:]])   # (NaN is the empty field)
                assert (text[:, 0] == np.arange(1, w.ncell + 1)).all()                 # ids from 1
                assert np.array_equal(text[:, 1:], got[0], equal_nan=True)             # the csv parses back to the npy exactly
    check(out, c.extremes)
    # a second run whose fit is the first run's: the return periods of a wetter run under the first run's climate
    tables = {(v, k): np.load(os.path.join(out, 'extremes_{}_{}_{}.npy'.format(v, k, PROJECT))) for v in VARS for k in ('max', 'min')}
    c2 = run_model(example(tmp_path / 'second', min_years=10, parameters=os.path.join(out, PROJECT)))
    out2 = os.path.join(str(tmp_path), 'second', 'output', PROJECT)
    for key, table in tables.items():
        assert c2.extremes[key]['table'][:, :8].tobytes() == table[:, :8].tobytes()
    check(out2, c2.extremes, parameters=tables)
