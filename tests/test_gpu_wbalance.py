"""xh_water_balance on the device: every kind of quadruple of tests/wbalance_cases.py at every year count against
the host build of the same header (tests/wbalance_probe), determinism, windows, lags, NULL inputs and outputs, the argument
errors, balance_rows on host and device arrays, and run_model with CalculateWaterBalance = 1 at cell and basin level.

Every column but omega and budyko_dev must be the host build's bits, and so must the annual totals and the cross-correlation;
those two come through the device's exp, log, log1p and expm1 and are held to the bounds of tests/test_wbalance_host.py -- 4 x
the distance measured for the restatement from 40-digit values (1.013e-14 relative for omega, 1.585e-15 of max(|value|, 1) for
budyko_dev), against those 40-digit values, on every row.  NaN masks are identical.  64 rows per call: the 15 kinds over and
over, one workgroup each."""
import os
import re

import numpy as np
import pytest

import wbalance_cases as cases
import wbalance_np as wnp
from test_wbalance_host import BIT_COLUMNS, bounded_columns, host_balance, probe, same_bits  # noqa: F401  (probe: the fixture)

pytestmark = pytest.mark.gpu
NROWS = 64
FILL = -7.0


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def device_balance(ctx, p, pet, q, aet=None, start=0, nyear=None, max_lag=cases.MAX_LAG, omega0=cases.OMEGA0, annual=True, xcorr=True,
                   fill=FILL):
    arrays = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (p, pet, q, aet)]
    nrows, stride = arrays[0].shape
    nyear = (stride - start) // 12 if nyear is None else nyear
    d_in = [None if a is None else ctx.upload(a) for a in arrays]
    d_t = ctx.upload(np.full((nrows + 1, wnp.NCOL), fill))                       # one row more of each: nothing is written past
    d_a, d_x = ctx.upload(np.full((nrows + 1, 4, nyear), fill)), ctx.upload(np.full((nrows + 1, max_lag + 1), fill))   # [nrows, ...]
    ctx.water_balance(nrows, stride, start, nyear, max_lag, omega0, d_in[0], d_in[1], d_in[2], d_in[3], d_t, d_a if annual else None,
                      d_x if xcorr else None)
    out = [d.download() for d in (d_t, d_a, d_x)]
    assert all((o[nrows:] == fill).all() for o in out)
    for a in d_in + [d_t, d_a, d_x]:
        if a is not None:
            a.free()
    return tuple(o[:nrows] for o in out)


def tiled(years):
    """64 rows of each array: the 15 kinds over and over; row i is kind i mod 15."""
    return tuple(a[np.arange(NROWS) % len(cases.KINDS)] for a in cases.rows(years))


def same(got, ref, tag):
    assert same_bits(got[0][:, BIT_COLUMNS], ref[0][:, BIT_COLUMNS]), tag
    assert same_bits(got[1], ref[1]) and same_bits(got[2], ref[2]), tag
    assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0])), tag


@pytest.mark.parametrize('years', cases.YEARS)
def test_every_kind_of_row_at_every_year_count(ctx, probe, golden, years):  # noqa: F811
    quad = tiled(years)
    for with_aet in (True, False):
        rows = quad if with_aet else quad[:3] + (None,)
        got = device_balance(ctx, *rows)
        same(got, host_balance(probe, *rows), 'device {} {}'.format(years, with_aet))
        for first in range(0, NROWS - len(cases.KINDS) + 1, len(cases.KINDS)):            # every copy of the 15 rows, none left out
            bounded_columns(golden, got[0][first:first + len(cases.KINDS)], years, with_aet, 'device {} rows {}..'.format(years, first))
        assert got[0][-1].tobytes() == got[0][NROWS - 1 - len(cases.KINDS)].tobytes()     # (the last, incomplete copy)
        # two calls give identical bytes
        again = device_balance(ctx, *rows, fill=3.0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_windows_strides_and_lags(ctx, probe):  # noqa: F811
    quad = tiled(22)
    wide = [np.concatenate([a[:, -7:], a, a[:, :10]], axis=1) for a in quad]
    for start, nyear, max_lag, omega0 in ((0, 22, 6, 2.6), (7, 22, 0, 2.6), (17, 21, 12, 1.5), (9, 12, 3, 4.0)):
        got = device_balance(ctx, *wide, start=start, nyear=nyear, max_lag=max_lag, omega0=omega0)
        assert got[2].shape == (NROWS, max_lag + 1) and got[1].shape == (NROWS, 4, nyear)
        ref = host_balance(probe, *wide, start=start, nyear=nyear, max_lag=max_lag, omega0=omega0)
        same(got, ref, 'window {} {} {}'.format(start, nyear, max_lag))
        with np.errstate(invalid='ignore'):                  # (no 40-digit values of these windows: that the columns are filled at all)
            assert not (np.abs(got[0][:, 11:13] - ref[0][:, 11:13]) > 1e-12 * np.maximum(np.abs(ref[0][:, 11:13]), 1.0)).any()


def test_null_outputs_are_left_alone(ctx):
    quad = tiled(33)
    full = device_balance(ctx, *quad)
    for annual, xcorr in ((False, True), (True, False), (False, False)):
        got = device_balance(ctx, *quad, annual=annual, xcorr=xcorr)
        assert got[0].tobytes() == full[0].tobytes()
        assert got[1].tobytes() == full[1].tobytes() if annual else (got[1] == FILL).all()
        assert got[2].tobytes() == full[2].tobytes() if xcorr else (got[2] == FILL).all()


def test_argument_errors_launch_nothing(ctx):
    from xanthos_amd import _hip
    d_x, d_t = ctx.upload(np.ones((2, 5000))), ctx.upload(np.full((2, wnp.NCOL), FILL))
    d_a, d_c = ctx.upload(np.full((2, 4, 341), FILL)), ctx.upload(np.full((2, 13), FILL))
    lib = _hip.lib()

    def refused(pattern, **bad):
        arg = dict(stride=130, col0=0, nyear=10, max_lag=6, omega0=2.6, p=d_x.ptr, pet=d_x.ptr, q=d_x.ptr, table=d_t.ptr)
        arg.update(bad)
        rc = lib.xh_water_balance(ctx.handle, 2, arg['stride'], arg['col0'], arg['nyear'], arg['max_lag'], arg['omega0'], arg['p'],
                                  arg['pet'], arg['q'], None, arg['table'], d_a.ptr, d_c.ptr)
        assert rc == 1, bad
        with pytest.raises(_hip.HipError) as exc:
            ctx._check(rc)
        assert 'error 1' in str(exc.value) and re.search(pattern, str(exc.value)), str(exc.value)
    refused(r'NULL array \(d_p (\(nil\)|0x0|0)', p=None)
    refused(r'NULL array .*d_pet (\(nil\)|0x0|0),', pet=None)
    refused(r'NULL array .*d_q (\(nil\)|0x0|0),', q=None)
    refused(r'NULL array .*d_table (\(nil\)|0x0|0)\)', table=None)
    refused(r'column -1', col0=-1)
    refused(r'column 11, 10 years = 120 columns', col0=11)
    refused(r'nyear \(0\)', nyear=0)
    refused(r'nyear \(342\)', nyear=342, stride=5000)
    refused(r'max_lag \(-1\)', max_lag=-1)
    refused(r'max_lag \(13\)', max_lag=13)
    refused(r'omega0 \(1\)', omega0=1.0)
    refused(r'omega0 \(0\.5\)', omega0=0.5)
    refused(r'omega0 \(-?nan\)', omega0=float('nan'))
    refused(r'omega0 \(inf\)', omega0=float('inf'))
    ctx.sync()
    assert (d_t.download() == FILL).all() and (d_a.download() == FILL).all() and (d_c.download() == FILL).all()
    before = ctx.timing('water_balance')[1]
    ctx.water_balance(2, 5000, 908, 341, 12, 2.6, d_x, d_x, d_x, None, d_t, d_a, d_c)   # the longest window there is, to the row's last column
    ctx.sync()
    assert ctx.timing('water_balance')[1] == before + 1                                # the timer's name
    out = d_t.download()
    assert (out[:, 0] == 341).all() and (out[:, 1] == 4092).all() and (out[:, [2, 3, 5]] == 12.0).all() and (out[:, [6, 7]] == 1.0).all()
    assert (out[:, 18] == 0.0).all() and np.isnan(out[:, [4, 8, 9, 10, 11, 13, 14, 15, 16, 17, 19, 20]]).all()
    ann = d_a.download()
    assert (ann[:, [0, 1, 3]] == 12.0).all() and np.isnan(ann[:, 2]).all() and np.isnan(d_c.download()).all()
    for a in (d_x, d_t, d_a, d_c):
        a.free()


def test_balance_rows_on_host_and_device_arrays(ctx, probe):  # noqa: F811
    from xanthos_amd import _hip, waterbalance
    quad = [a[:40] for a in tiled(21)]
    host = waterbalance.balance_rows(ctx, *quad)
    d_quad = [ctx.upload(a) for a in quad]
    dev = waterbalance.balance_rows(ctx, *d_quad)
    assert all(isinstance(a, _hip.DeviceArray) for a in host) and [tuple(a.shape) for a in host] == [(40, 21), (40, 4, 21), (40, 7)]
    a, b = [x.download() for x in host], [x.download() for x in dev]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    same(a, host_balance(probe, *quad), 'balance_rows')
    win = waterbalance.balance_rows(ctx, d_quad[0], quad[1], d_quad[2], None, start=24, nyear=10, max_lag=2, omega0=1.9)
    same([x.download() for x in win], host_balance(probe, quad[0], quad[1], quad[2], None, 24, 10, 2, 1.9), 'balance_rows window')
    # an observed basin series with gaps is a host array like any other
    gap = np.where(np.arange(252) % 7 == 0, np.nan, quad[2][:1])
    obs = waterbalance.balance_rows(ctx, quad[0][:1], quad[1][:1], gap)
    t = obs[0].download()
    assert t[0, 1] == 216 and t[0, 0] == 0 and same_bits(t[:, BIT_COLUMNS], wnp.water_balance(quad[0][:1], quad[1][:1], gap)[0][:, BIT_COLUMNS])
    with pytest.raises(ValueError, match='one shape'):
        waterbalance.balance_rows(ctx, quad[0], quad[1][:, :-12], quad[2])
    with pytest.raises(_hip.HipError, match='omega0'):
        waterbalance.balance_rows(ctx, *d_quad, omega0=1.0)
    for x in host + dev + win + obs + tuple(d_quad):
        x.free()


# ------------------------------------------------------------------ run_model
PROJECT = 'pm_abcd_mrtm_synth'
YEARS = (1971, 1982)
NPY = 4


def files_of(folder, skip=('logfile.log',)):
    out = {}
    for base, _, names in os.walk(folder):
        for f in names:
            if f not in skip:
                out[os.path.relpath(os.path.join(base, f), folder)] = os.path.join(base, f)
    return out


def test_run_model_writes_the_water_balance_and_nothing_else_changes(tmp_path, golden):
    import filecmp
    from xanthos_amd import run_model, synth
    w = synth.make_world(nrow=48, ncol=96, ncell=2000, n_basins=8, seed=21)
    nm = 12 * (YEARS[1] - YEARS[0] + 1)
    forcing = synth.make_forcing(w, nm, seed=100)

    def example(root, on):
        ini = synth.write_example(str(root), w, forcing, YEARS[0], YEARS[1], runoff_spinup=25, routing_spinup=6,
                                  output_vars=('q', 'pet', 'aet'), output_format=NPY)
        if on:
            synth.with_water_balance(ini, levels=('cell', 'basin'), year_start_month=10, annual=1)
        return ini
    run_model(example(tmp_path / 'plain', False))
    c = run_model(example(tmp_path / 'balance', True))
    out_plain, out = [os.path.join(str(tmp_path), d, 'output', PROJECT) for d in ('plain', 'balance')]
    fa, fb = files_of(out_plain), {k: v for k, v in files_of(out).items() if not k.startswith('water_balance_')}
    assert sorted(fa) == sorted(fb) and fa
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), rel                     # every other file byte for byte
    names = ['water_balance_{}{}_{}.{}'.format(level, what, PROJECT, e) for level in ('cell', 'basin')
             for what, e in (('', 'npy'), ('', 'csv'), ('_xcorr', 'npy'), ('_annual', 'npy'))]
    assert sorted(k for k in files_of(out) if k.startswith('water_balance_')) == sorted(names)
    # years from October: 1971/72 .. 1981/82, the last one ending with the run's last month
    m0, nyear = 9, 11
    assert sorted(c.water_balance) == ['basin', 'cell']
    q, pet, aet = (np.load(os.path.join(out, '{}_{}.npy'.format(name, PROJECT))) for name in ('q_mmpermonth', 'pet_mmpermonth', 'aet_mmpermonth'))
    precip = np.asarray(forcing['precip'], dtype=np.float64)
    assert q.shape == precip.shape == (w.ncell, nm)
    # the basin rows in xh_agg_spatial's order: x area x 1e-6 per cell, then a plain sum over ascending cells from 0.0, NaN skipped
    scale = np.asarray(c.data.area, dtype=np.float64) * 1e-6                    # (the loader's km2: the file holds ha)
    ids = np.asarray(c.data.basin_ids)

    def basin(x):
        rows = np.full((8, nm), np.nan)
        for b in range(8):
            cells = np.nonzero(ids == b + 1)[0]
            if cells.size:
                acc = np.zeros(nm)
                for cell in cells:
                    v = x[cell] * scale[cell]
                    acc = np.where(np.isnan(v), acc, acc + v)
                rows[b] = acc
        return rows
    inputs = {'cell': (precip, pet, q, aet), 'basin': tuple(basin(x) for x in (precip, pet, q, aet))}
    for level, n in (('cell', w.ncell), ('basin', 8)):
        want = wnp.water_balance(*inputs[level], start=m0, nyear=nyear, max_lag=6, omega0=2.6)
        stem = os.path.join(out, 'water_balance_' + level)
        got = (np.load('{}_{}.npy'.format(stem, PROJECT)), np.load('{}_annual_{}.npy'.format(stem, PROJECT)),
               np.load('{}_xcorr_{}.npy'.format(stem, PROJECT)))
        assert got[0].shape == (n, 21) and got[1].shape == (n, 4, nyear) and got[2].shape == (n, 7)
        same(got, want, 'run_model ' + level)
        # omega and budyko_dev against the restatement, which lies within 2.532e-15 and 3.963e-16 of 40-digit values on the case
        # rows: the case rows' bounds (4 x those, against the 40-digit values) plus the restatement's own distance
        dist = golden('wbalance')['dist_table']
        with np.errstate(invalid='ignore'):
            assert not (np.abs(got[0][:, 11] - want[0][:, 11]) > 5.0 * dist[11] * np.abs(want[0][:, 11])).any()
            assert not (np.abs(got[0][:, 12] - want[0][:, 12]) > 5.0 * dist[12] * np.maximum(np.abs(want[0][:, 12]), 1.0)).any()
        res = c.water_balance[level]
        assert all(res[k].tobytes() == a.tobytes() for k, a in zip(('table', 'annual', 'xcorr'), got))
        assert (got[0][:, 0] == nyear).sum() > n // 2 and (~np.isnan(got[0][:, 11])).sum() > n // 4
        unit = 'mm' if level == 'cell' else 'km3'
        header = 'id,' + ','.join(c_ + '_' + unit if c_.endswith('_mean') else c_ for c_ in wnp.COLUMNS)
        lines = open('{}_{}.csv'.format(stem, PROJECT)).read().splitlines()
        assert lines[0] == header and len(lines) == n + 1
        text = np.array([[float(v or 'nan') for v in ln.split(',')] for ln in lines[1:]])   # (NaN is the empty field)
        assert (text[:, 0] == np.arange(1, n + 1)).all()                       # ids from 1
        assert np.array_equal(text[:, 1:], got[0], equal_nan=True)             # the csv parses back to the npy exactly
