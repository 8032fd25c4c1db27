"""xh_trend on the device: the rows of tests/trend_cases.py at every shape against the numpy restatement
(tests/trend_np.py) and against the host build of the same header (tests/trend_probe), determinism, a window inside a longer
row, the argument errors, trend_rows on host and device arrays, and run_model with CalculateTrend = 1.

Nine columns must EQUAL the restatement's (==; identical NaN masks): integers, correctly rounded operations and exact order
statistics leave no room.  p = erfc(|z| / sqrt 2) comes from the device's erfc, another implementation than the host's: it is
held to the bound of tests/test_trend_host.py -- 4 x the error measured for scipy's erfc against 40-digit values on these rows,
7.099e-14, so 2.84e-13 relative --, and where the restatement's p lies below 2.3e-308 (the strictly monotone seasonal rows of
64 and more years, z > 40) to 0 <= p <= 2.3e-308.

300 rows per call, more than one workgroup per CU.  All 300 are different rows, except at 12 x 257 columns, where the
restatement sorts 395,000 slopes per row: there 72 different rows (every kind six times) are laid out 300 times, row r a copy
of row r mod 72, so that every workgroup is still held against the restatement."""
import os
import re

import numpy as np
import pytest

import trend_cases as cases
import trend_np
from test_trend_host import host_trend, p_bound, probe  # noqa: F401  (probe: the fixture)

pytestmark = pytest.mark.gpu
NROWS = 300
DISTINCT_AT_THE_LARGEST = 72


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def device_trend(ctx, rows, nseason, z_conf=cases.Z95, start=0, ncol=None, fill=-7.0):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ncol = rows.shape[1] - start if ncol is None else ncol
    d_x, d_out = ctx.upload(rows), ctx.upload(np.full((rows.shape[0], 10), fill))
    ctx.trend(rows.shape[0], rows.shape[1], start, ncol, nseason, z_conf, d_x, d_out)
    out = d_out.download()
    d_x.free()
    d_out.free()
    return out


def rows_of(nseason, years):
    if (nseason, years) == (12, 257):
        base = cases.make_rows(nseason, years, DISTINCT_AT_THE_LARGEST)
        return base[np.arange(NROWS) % DISTINCT_AT_THE_LARGEST], DISTINCT_AT_THE_LARGEST
    return cases.make_rows(nseason, years, NROWS), NROWS


def held(got, ref, bound, tag):
    assert cases.same_but_p(got, ref), (tag, np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:10])
    ok = ~np.isnan(ref[:, 4]) & (ref[:, 4] >= cases.TINY)
    err = float((np.abs(got[ok, 4] - ref[ok, 4]) / ref[ok, 4]).max()) if ok.any() else 0.0
    print('{}: p max relative error {:.3e} (bound {:.3e})'.format(tag, err, bound))
    assert cases.p_within(got[:, 4], ref[:, 4], bound), (tag, err)


@pytest.mark.parametrize('nseason,years', cases.SHAPES)
def test_every_kind_of_row_at_every_shape(ctx, probe, golden, nseason, years):  # noqa: F811
    bound = p_bound(golden)
    rows, distinct = rows_of(nseason, years)
    got = device_trend(ctx, rows, nseason)
    ref = trend_np.trend_rows(rows[:distinct], nseason, cases.Z95)[np.arange(NROWS) % distinct]
    held(got, ref, bound, '{} x {}'.format(nseason, years))
    monotone = np.array([cases.KINDS[(r % distinct) % len(cases.KINDS)] in ('increasing', 'decreasing') for r in range(NROWS)])
    tiny = ~np.isnan(ref[:, 4]) & (ref[:, 4] < cases.TINY)
    assert np.array_equal(tiny, monotone & (nseason == 12 and years >= 64))
    # the host build of the same header: all ten columns bit for bit but p
    host = host_trend(probe, rows[:cases.HOST_ROWS], nseason)
    cols = [c for c in range(10) if c != 4]
    assert got[:cases.HOST_ROWS][:, cols].tobytes() == host[:, cols].tobytes()
    # two calls give identical bits
    assert device_trend(ctx, rows, nseason, fill=3.0).tobytes() == got.tobytes()


def test_window_inside_a_longer_row(ctx, golden):
    bound = p_bound(golden)
    rng = np.random.default_rng(5)
    wide = rng.normal(size=(NROWS, 12 * 30 + 17))
    wide[2, 40:90] = np.nan
    wide[5::7, 100] = np.inf
    for nseason, start, ncol in ((12, 5, 12 * 22), (1, 3, 65), (4, 17, 4 * 65), (12, 17, 12 * 30)):
        got = device_trend(ctx, wide, nseason, start=start, ncol=ncol)
        held(got, trend_np.trend_rows(wide, nseason, cases.Z95, start, ncol), bound, 'window {} {} {}'.format(nseason, start, ncol))
    other = device_trend(ctx, wide, 12, z_conf=-0.8416212335729143, start=5, ncol=12 * 22)
    held(other, trend_np.trend_rows(wide, 12, -0.8416212335729143, 5, 12 * 22), bound, 'confidence 0.6')


def test_argument_errors_launch_nothing(ctx):
    from xanthos_amd import _hip
    d_x, d_out = ctx.upload(np.ones((2, 4200))), ctx.upload(np.full((2, 10), -7.0))
    lib = _hip.lib()

    def refused(code, pattern, rc):
        assert rc == code
        with pytest.raises(_hip.HipError) as exc:
            ctx._check(rc)
        assert 'error {}'.format(code) in str(exc.value) and re.search(pattern, str(exc.value)), str(exc.value)
    call = lambda stride, col0, ncol, ns, z, x=d_x.ptr, out=d_out.ptr: lib.xh_trend(ctx.handle, 2, stride, col0, ncol, ns, z, x, out)
    refused(1, 'NULL', call(24, 0, 24, 12, -1.96, x=None))
    refused(1, 'NULL', call(24, 0, 24, 12, -1.96, out=None))
    refused(1, r'column -1', call(24, -1, 12, 12, -1.96))
    refused(1, r'column 13, 12 columns', call(24, 13, 12, 12, -1.96))
    refused(1, r'0 columns', call(24, 0, 0, 1, -1.96))
    refused(1, r'no multiple of nseason', call(24, 0, 20, 12, -1.96))
    for z in (1.96, 0.0, float('nan'), float('-inf')):
        refused(1, 'z_conf', call(24, 0, 24, 12, z))
    refused(3, '4096', call(4200, 0, 4097, 1, -1.96))
    refused(3, r'nseason \(0\)', call(24, 0, 24, 0, -1.96))
    refused(3, r'nseason \(13\)', call(26, 0, 26, 13, -1.96))
    ctx.sync()
    assert (d_out.download() == -7.0).all()
    before = ctx.timing('trend')[1]
    ctx.trend(2, 4200, 104, 4096, 1, -1.96, d_x, d_out)          # the longest row there is
    ctx.sync()
    assert ctx.timing('trend')[1] == before + 1                  # the timer's name
    out = d_out.download()
    assert (out[:, [0, 9]] == [4096.0, 4096 * 4095 / 2]).all() and (out[:, [1, 2, 3, 5, 7, 8]] == 0.0).all() and (out[:, 4] == 1.0).all()
    assert (out[:, 6] == 1.0).all()
    d_x.free()
    d_out.free()


def test_trend_rows_on_host_and_device_arrays(ctx, golden):
    from xanthos_amd import _hip, trend
    rows = cases.make_rows(12, 22, 40)
    t_host = trend.trend_rows(ctx, rows, nseason=12)
    d_rows = ctx.upload(rows)
    t_dev = trend.trend_rows(ctx, d_rows, nseason=12)
    assert isinstance(t_host, _hip.DeviceArray) and tuple(t_host.shape) == (40, 10)
    a, b = t_host.download(), t_dev.download()
    assert a.tobytes() == b.tobytes()
    held(a, trend_np.trend_rows(rows, 12, trend.z_of(0.95)), p_bound(golden), 'trend_rows')
    t_win = trend.trend_rows(ctx, d_rows, nseason=1, start=7, ncol=64, confidence=0.9)
    held(t_win.download(), trend_np.trend_rows(rows, 1, trend.z_of(0.9), 7, 64), p_bound(golden), 'trend_rows window')
    with pytest.raises(ValueError, match='confidence'):
        trend.trend_rows(ctx, d_rows, confidence=1.0)
    with pytest.raises(_hip.HipError, match='nseason'):
        trend.trend_rows(ctx, d_rows, nseason=13)
    for a in (t_host, t_dev, t_win, d_rows):
        a.free()


# ------------------------------------------------------------------ run_model
PROJECT = 'pm_abcd_mrtm_synth'
YEARS = (1971, 1976)
WINDOW = (1972, 1976)
NPY = 4


def files_of(folder, skip=('logfile.log',)):
    out = {}
    for base, _, names in os.walk(folder):
        for f in names:
            if f not in skip:
                out[os.path.relpath(os.path.join(base, f), folder)] = os.path.join(base, f)
    return out


def test_run_model_writes_the_tables_and_nothing_else_changes(tmp_path, golden):
    import filecmp
    from oracle import writer as o_writer
    from xanthos_amd import run_model, synth
    bound = p_bound(golden)
    w = synth.make_world(nrow=36, ncol=72, ncell=300, n_basins=3, seed=21)
    nm = 12 * (YEARS[1] - YEARS[0] + 1)
    forcing = synth.make_forcing(w, nm, seed=100)

    def example(root, with_trend):
        ini = synth.write_example(str(root), w, forcing, YEARS[0], YEARS[1], runoff_spinup=25, routing_spinup=6,
                                  output_vars=('q', 'avgchflow', 'soilmoisture'), output_format=NPY)
        if with_trend:
            synth.enable_trend(ini, trend_vars=('q', 'avgchflow'), series=('annual', 'seasonal'), start_year=WINDOW[0],
                               end_year=WINDOW[1])
        return ini
    run_model(example(tmp_path / 'plain', False))
    c = run_model(example(tmp_path / 'trend', True))
    out_plain, out = [os.path.join(str(tmp_path), d, 'output', PROJECT) for d in ('plain', 'trend')]
    fa, fb = files_of(out_plain), {k: v for k, v in files_of(out).items() if not k.startswith('trend_')}
    assert sorted(fa) == sorted(fb) and fa
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), rel                     # every other file byte for byte
    assert sorted(k for k in files_of(out) if k.startswith('trend_')) == sorted(
        'trend_{}_{}_{}.{}'.format(v, s, PROJECT, e) for v in ('q', 'avgchflow') for s in ('annual', 'seasonal') for e in ('npy', 'csv'))
    written = {'q': np.load(os.path.join(out, 'q_mmpermonth_{}.npy'.format(PROJECT))),
               'avgchflow': np.load(os.path.join(out, 'avgchflow_m3persec_{}.npy'.format(PROJECT)))}
    m0, z_conf = 12 * (WINDOW[0] - YEARS[0]), -1.9599639845400536
    nyr = WINDOW[1] - WINDOW[0] + 1
    assert sorted(c.trend) == sorted((v, s) for v in ('q', 'avgchflow') for s in ('annual', 'seasonal'))
    for var, x in written.items():
        assert x.shape == (w.ncell, nm)
        # the year as the section's default forms it: np.sum of the 12 months for q, pandas' mean for avgchflow
        yearly = x.reshape(w.ncell, -1, 12).sum(axis=2) if var == 'q' else o_writer.agg_to_year(x, 'mean')
        want = {'annual': trend_np.trend_rows(yearly, 1, z_conf, WINDOW[0] - YEARS[0], nyr),
                'seasonal': trend_np.trend_rows(x, 12, z_conf, m0, 12 * nyr)}
        for series in ('annual', 'seasonal'):
            stem = os.path.join(out, 'trend_{}_{}_{}'.format(var, series, PROJECT))
            table = np.load(stem + '.npy')
            assert table.shape == (w.ncell, 10)
            held(table, want[series], bound, 'run_model {} {}'.format(var, series))
            assert (table[:, 0] == (nyr if series == 'annual' else 12 * nyr)).all() and not np.isnan(table).any()
            assert table.tobytes() == c.trend[(var, series)].tobytes()
            lines = open(stem + '.csv').read().splitlines()
            assert lines[0] == 'id,' + ','.join(trend_np.COLUMNS) and len(lines) == w.ncell + 1
            text = np.array([[float(v) for v in ln.split(',')] for ln in lines[1:]])
            assert (text[:, 0] == np.arange(1, w.ncell + 1)).all()                 # ids from 1
            assert text[:, 1:].tobytes() == table.tobytes()                        # the csv parses back to the npy exactly
