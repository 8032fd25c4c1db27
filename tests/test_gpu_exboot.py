"""xh_extremes_boot on the device: the 300 rows of tests/extremes_cases.py and the sparse rows of
tests/exboot_cases.py at the shapes DEVICE_SHAPES and both kinds against the host build of the same header
(tests/exboot_probe), determinism, the row0 / slice and the B-prefix property, windows, a NULL d_rep, the argument errors,
bootstrap_rows on host and device arrays, and run_model with ``bootstrap`` in [Extremes].

Every replicate's l1, l2, t3, t4 and nb must be the host build's bits; k*, the levels and every bound come through the device's
expm1, log and tgamma and are held to the bounds of tests/test_exboot_host.py -- 4 x the error measured for the restatement
against 40-digit values, per quantity and class; the NaN masks are identical; and the bounds are np.quantile of the device's
own replicate values, bit for bit.  348 rows per call: 348 one-wavefront workgroups; test_more_rows_than_workgroups runs 5,220
rows on the 2,048 workgroups the grid is capped at, and test_the_largest_workgroup 341 years with 2,048 replicates."""
import os
import re

import numpy as np
import pytest

import exboot_cases as xc
import exboot_np
import extremes_cases as cases
import extremes_np
from test_exboot_host import T, bprobe, held, host_exboot  # noqa: F401  (bprobe: the fixture)

pytestmark = pytest.mark.gpu
NROWS = 300
FILL = -7.0


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def device_exboot(ctx, rows, kind, B, periods=T, confidence=xc.CONFIDENCE, seed=xc.SEED, row0=0, min_years=cases.MIN_YEARS, start=0,
                  nyear=None, rep=True, fill=FILL):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    nyear = (rows.shape[1] - start) // 12 if nyear is None else nyear
    d_x = ctx.upload(rows)
    d_ci = ctx.upload(np.full((rows.shape[0], 3 + 2 * len(periods)), fill))
    d_rep = ctx.upload(np.full((rows.shape[0], B, 5 + len(periods)), fill))
    ctx.extremes_boot(rows.shape[0], rows.shape[1], start, nyear, kind, min_years, periods, B, confidence, seed, d_x, d_ci,
                      d_rep if rep else None, row0)
    out = d_ci.download(), d_rep.download()
    for a in (d_x, d_ci, d_rep):
        a.free()
    return out


def table_of(rows, kind, start=0, nyear=None):
    return extremes_np.extremes_rows(rows, kind, (), min_years=cases.MIN_YEARS, start=start, nyear=nyear)[0]


@pytest.mark.parametrize('kind', extremes_np.KINDS)
@pytest.mark.parametrize('years,B', xc.DEVICE_SHAPES)
def test_every_kind_of_row_at_every_shape(ctx, bprobe, golden, years, B, kind):  # noqa: F811
    rows = xc.make_rows(years, NROWS)
    got = device_exboot(ctx, rows, kind, B)
    ref = host_exboot(bprobe, rows, kind, B)
    held(golden, got, ref, table_of(rows, kind), NROWS, 'device {} {} {}'.format(years, B, kind))
    have = ~np.isnan(got[0][:, 1])
    assert have[:NROWS].sum() > NROWS // 3 and (~have[:NROWS]).sum() > NROWS // 10
    assert np.array_equal(have, (2 * got[0][:, 0] >= B) & (got[0][:, 0] > 0))
    # the bounds are numpy's quantile of the device's own replicate values, bit for bit
    for r in np.flatnonzero(have):
        assert xc.same_bits(got[0][r], exboot_np.intervals(got[1][r], B, xc.CONFIDENCE, kind)), (years, B, kind, r)
    assert (got[0][have, 1::2] <= got[0][have, 2::2]).all()
    # two calls give identical bytes
    again = device_exboot(ctx, rows, kind, B, fill=3.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize('years,B,kind', ((10, 65, 'max'), (5, 64, 'min')))
def test_more_rows_than_workgroups(ctx, bprobe, golden, years, B, kind):  # noqa: F811
    """5,220 rows on a grid capped at 8 workgroups per CU (2,048 on 256 CUs): every workgroup walks two or three rows, one after
    another in the same LDS and the same slab.  Against the host build (the sums and nb bit for bit, the rest in its bounds), and
    the same bytes as the rows computed in slices of fewer rows than workgroups with row0 -- the result does not depend on the
    grid."""
    base = xc.make_rows(years, NROWS)
    rows = np.tile(base, (15, 1))                                                        # (every row number draws anew)
    assert rows.shape[0] == 5220 > 2 * xc.GRID_CAP and ctx.cu_count() * 8 <= xc.GRID_CAP
    shifted = np.array([xc.row_class(r % base.shape[0], NROWS) == 'shifted' for r in range(rows.shape[0])])
    got = device_exboot(ctx, rows, kind, B)
    ref = host_exboot(bprobe, rows, kind, B)
    held(golden, got, ref, table_of(rows, kind), shifted, 'beyond the grid {} {} {}'.format(years, B, kind))
    for a in range(0, rows.shape[0], 1500):
        part = device_exboot(ctx, rows[a:a + 1500], kind, B, row0=a)
        assert part[0].tobytes() == got[0][a:a + 1500].tobytes() and part[1].tobytes() == got[1][a:a + 1500].tobytes(), a
    # the rows differ by their number alone: the same series at another place draws other replicates
    assert not xc.same_bits(got[1][:base.shape[0]], got[1][base.shape[0]:2 * base.shape[0]])


def test_the_largest_workgroup(ctx, bprobe, golden):  # noqa: F811
    """341 years with 2,048 replicates: 74,056 B of LDS, asked for beyond the 64 KB a kernel gets unasked, a 2,048-wide sort over
    the stage's memory and the largest slab, on rows with a fit (and one of each kind without)."""
    rows = xc.make_rows(341, 15)[[0, 1, 3, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 56, 60]]
    got = device_exboot(ctx, rows, 'max', 2048)
    ref = host_exboot(bprobe, rows, 'max', 2048)
    assert (ref[0][:, 0] > 0).sum() >= 10 and (ref[0][:, 0] == 0).sum() >= 3
    assert cases.kind_of(12) == 'shifted'                                             # (row 12 of make_rows, the tenth here)
    held(golden, got, ref, table_of(rows, 'max'), np.arange(15) == 9, 'the largest workgroup')
    again = device_exboot(ctx, rows, 'max', 2048, fill=3.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_the_halving_rule_on_the_device(ctx):
    """The sparse rows at B = 2 and 64: some 'two' rows have nb < B / 2 -- nb reported, every bound NaN -- and most have not
    (tests/test_exboot_host.py pins the same on the host)."""
    for years, B in ((10, 2), (341, 64), (63, 65)):
        ci = device_exboot(ctx, xc.sparse_rows(years), 'max', B, row0=NROWS, rep=False)[0]
        two = ci[:xc.TWO_ROWS]
        under = np.isnan(two[:, 1])
        assert np.array_equal(under, 2 * two[:, 0] < B) and np.isnan(two[under, 1:]).all() and not np.isnan(two[~under]).any()
        assert 1 <= under.sum() <= 20 and ((two[under, 0] > 0).any() or B == 2), (years, B, two[:, 0])


def test_slices_of_rows_prefixes_of_replicates_and_seeds(ctx):
    rows = xc.make_rows(50, 100)
    small, large = device_exboot(ctx, rows, 'max', 64), device_exboot(ctx, rows, 'max', 130)
    assert xc.same_bits(small[1], large[1][:, :64]) and not xc.same_bits(small[0], large[0])
    for a, b in ((0, 1), (7, 19), (99, 148)):
        part = device_exboot(ctx, rows[a:b], 'max', 64, row0=a)
        assert part[0].tobytes() == small[0][a:b].tobytes() and part[1].tobytes() == small[1][a:b].tobytes(), (a, b)
    assert not xc.same_bits(device_exboot(ctx, rows[7:19], 'max', 64)[1], small[1][7:19])
    other = device_exboot(ctx, rows, 'max', 64, seed=xc.SEED + 1)
    assert not xc.same_bits(other[1], small[1]) and np.array_equal(other[0][:, 0] > 0, small[0][:, 0] > 0)
    # a row number beyond 2^31
    far = device_exboot(ctx, rows[:4], 'min', 64, row0=2 ** 31 + 5)
    assert xc.same_bits(far[1][:, :, :4], exboot_np.bootstrap_rows(rows[:4], 'min', T, 64, xc.CONFIDENCE, xc.SEED, row0=2 ** 31 + 5,
                                                                    min_years=cases.MIN_YEARS)[1][:, :, :4])


def test_windows_strides_and_numbers_of_periods(ctx, bprobe, golden):  # noqa: F811
    wide = xc.make_rows(30, NROWS)
    wide = np.concatenate([wide[:, -7:], wide, wide[:, :10]], axis=1)
    for start, nyear, periods in ((0, 30, (2.0,)), (7, 30, (1.5, 2, 5, 10, 20, 50, 100, 500)), (17, 29, ()), (9, 12, (10.0, 3.0))):
        for kind in extremes_np.KINDS:
            got = device_exboot(ctx, wide, kind, 70, periods=periods, start=start, nyear=nyear)
            assert got[0].shape == (wide.shape[0], 3 + 2 * len(periods)) and got[1].shape == (wide.shape[0], 70, 5 + len(periods))
            ref = host_exboot(bprobe, wide, kind, 70, periods=periods, start=start, nyear=nyear)
            held(golden, got, ref, table_of(wide, kind, start, nyear), NROWS, 'window {} {} {}'.format(start, nyear, kind))
    a = device_exboot(ctx, wide, 'max', 70, start=7, nyear=12, min_years=13)
    assert (a[0][:, 0] == 0).all() and np.isnan(a[0][:, 1:]).all() and np.isnan(a[1]).all()
    # another confidence: other bounds from the same replicates
    b90, b50 = device_exboot(ctx, wide, 'max', 70, nyear=30), device_exboot(ctx, wide, 'max', 70, nyear=30, confidence=0.5)
    have = ~np.isnan(b90[0][:, 1])
    assert b90[1].tobytes() == b50[1].tobytes() and (b90[0][have, 1] <= b50[0][have, 1]).all() and (b50[0][have, 2] <= b90[0][have, 2]).all()


def test_null_replicates_leave_the_bounds_alone(ctx):
    for years, B in ((64, 100), (341, 1000)):
        rows = xc.make_rows(years, 60)
        full = device_exboot(ctx, rows, 'max', B)
        got = device_exboot(ctx, rows, 'max', B, rep=False)
        assert got[0].tobytes() == full[0].tobytes() and (got[1] == FILL).all()


def test_argument_errors_launch_nothing(ctx):
    from xanthos_amd import _hip
    d_x, d_ci = ctx.upload(np.ones((2, 5000))), ctx.upload(np.full((2, 7), FILL))
    d_rep = ctx.upload(np.full((2, 2048, 7), FILL))
    lib = _hip.lib()
    periods = np.array([2.0, 10.0])
    before = ctx.timing('extremes_boot')[1]

    def refused(pattern, **bad):
        arg = dict(stride=130, col0=0, nyear=10, kind=0, min_years=5, nT=2, T=periods, B=100, confidence=0.9, row0=0, x=d_x.ptr, ci=d_ci.ptr)
        arg.update(bad)
        rc = lib.xh_extremes_boot(ctx.handle, 2, arg['stride'], arg['col0'], arg['nyear'], arg['kind'], arg['min_years'], arg['nT'],
                                  None if arg['T'] is None else arg['T'].ctypes.data, arg['B'], arg['confidence'], 1, arg['row0'],
                                  arg['x'], arg['ci'], d_rep.ptr)
        assert rc == 1, bad
        with pytest.raises(_hip.HipError) as exc:
            ctx._check(rc)
        assert 'error 1' in str(exc.value) and 'xh_extremes_boot' in str(exc.value) and re.search(pattern, str(exc.value)), str(exc.value)
    refused('NULL', x=None)
    refused('NULL', ci=None)
    refused('NULL return periods', T=None)
    refused(r'column -1', col0=-1)
    refused(r'column 11, 10 years = 120 columns', col0=11)
    refused(r'nyear \(0\)', nyear=0)
    refused(r'nyear \(342\)', nyear=342, stride=5000)
    refused(r'nT \(-1\)', nT=-1)
    refused(r'nT \(9\)', nT=9)
    refused(r'return period 1 \(1\)', T=np.array([2.0, 1.0]))
    refused(r'kind \(2\)', kind=2)
    refused(r'min_years \(4\)', min_years=4)
    refused(r'B \(1\)', B=1)
    refused(r'B \(2049\)', B=2049)
    refused(r'B \(-3\)', B=-3)
    refused(r'confidence \(0\)', confidence=0.0)
    refused(r'confidence \(1\)', confidence=1.0)
    refused(r'confidence \(nan\)', confidence=float('nan'))
    refused(r'row0 \(-1\)', row0=-1)
    ctx.sync()
    assert (d_ci.download() == FILL).all() and (d_rep.download() == FILL).all()
    assert ctx.timing('extremes_boot')[1] == before                                 # nothing was launched
    ctx.extremes_boot(2, 5000, 908, 341, 'max', 5, periods, 2048, 0.9, 1, d_x, d_ci, d_rep)      # the longest window and the most replicates
    ctx.sync()
    assert ctx.timing('extremes_boot')[1] == before + 1                             # the timer's name
    assert (d_ci.download()[:, 0] == 0).all() and np.isnan(d_ci.download()[:, 1:]).all() and np.isnan(d_rep.download()).all()
    for a in (d_x, d_ci, d_rep):
        a.free()


def test_bootstrap_rows_on_host_and_device_arrays(ctx, bprobe, golden):  # noqa: F811
    from xanthos_amd import _hip, extremes
    rows = xc.make_rows(50, 40)
    host = extremes.bootstrap_rows(ctx, rows, 'min', min_years=5, B=100, seed=xc.SEED)
    d_rows = ctx.upload(rows)
    dev = extremes.bootstrap_rows(ctx, d_rows, 'min', min_years=5, B=100, seed=xc.SEED, replicates=True)
    assert isinstance(host, _hip.DeviceArray) and tuple(host.shape) == (88, 15) and [tuple(a.shape) for a in dev] == [(88, 15), (88, 100, 11)]
    a, b = host.download(), [x.download() for x in dev]
    assert a.tobytes() == b[0].tobytes()
    ref = host_exboot(bprobe, rows, 'min', 100, periods=extremes.RETURN_PERIODS)
    held(golden, b, ref, table_of(rows, 'min'), 40, 'bootstrap_rows')
    win = extremes.bootstrap_rows(ctx, rows[10:30], 'max', 24, 20, (10.0,), 5, 64, 0.8, 3, 10)        # (the arguments in their order)
    ref = host_exboot(bprobe, rows[10:30], 'max', 64, periods=(10.0,), confidence=0.8, seed=3, row0=10, start=24, nyear=20, rep=False)
    held(golden, (win.download(), None), (ref[0], None), table_of(rows[10:30], 'max', 24, 20), 0, 'bootstrap_rows window')
    with pytest.raises(ValueError, match='kind'):
        extremes.bootstrap_rows(ctx, d_rows, 'mean')
    with pytest.raises(_hip.HipError, match=r'B \(3000\)'):
        extremes.bootstrap_rows(ctx, d_rows, 'max', B=3000)
    for x in (host, win, d_rows) + dev:
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


def test_run_model_writes_the_intervals_and_nothing_else_changes(tmp_path, golden):
    import filecmp
    from xanthos_amd import run_model, synth
    w = synth.make_world(nrow=48, ncol=96, ncell=2000, n_basins=8, seed=21)
    nm = 12 * (YEARS[1] - YEARS[0] + 1)
    forcing = synth.make_forcing(w, nm, seed=100)

    def example(root, **keys):
        ini = synth.write_example(str(root), w, forcing, YEARS[0], YEARS[1], runoff_spinup=25, routing_spinup=6,
                                  output_vars=('q', 'avgchflow', 'soilmoisture'), output_format=NPY)
        synth.enable_extremes(ini, extreme_vars=('q', 'avgchflow'), kinds=('max', 'min'), return_periods=PERIODS, year_start_month=10,
                              min_years=10, **keys)
        return ini
    c0 = run_model(example(tmp_path / 'plain'))
    c = run_model(example(tmp_path / 'boot', bootstrap=100, bootstrap_seed=7))
    out_plain, out = [os.path.join(str(tmp_path), d, 'output', PROJECT) for d in ('plain', 'boot')]
    fa, fb = files_of(out_plain), {k: v for k, v in files_of(out).items() if '_ci_' not in k}
    assert sorted(fa) == sorted(fb) and fa and not any('_ci_' in k for k in fa)
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), rel                     # every other file byte for byte
    names = ['extremes_{}_{}_ci_{}.{}'.format(v, k, PROJECT, e) for v in VARS for k in ('max', 'min') for e in ('npy', 'csv')]
    assert sorted(k for k in files_of(out) if '_ci_' in k) == sorted(names)
    assert all('ci' not in res for res in c0.extremes.values()) and sorted(c.extremes) == sorted(c0.extremes)
    m0, nyear = 9, 11
    for var, name in VARS.items():
        x = np.load(os.path.join(out, '{}_{}.npy'.format(name, PROJECT)))               # the run's own output array
        for kind in ('max', 'min'):
            stem = os.path.join(out, 'extremes_{}_{}_ci_{}'.format(var, kind, PROJECT))
            got = np.load(stem + '.npy')
            assert got.shape == (w.ncell, 3 + 2 * len(PERIODS)) and c.extremes[(var, kind)]['ci'].tobytes() == got.tobytes()
            assert c.extremes[(var, kind)]['table'].tobytes() == c0.extremes[(var, kind)]['table'].tobytes()
            want = exboot_np.bootstrap_rows(x, kind, PERIODS, 100, 0.90, 7, min_years=10, start=m0, nyear=nyear)[0]
            table = extremes_np.extremes_rows(x, kind, (), min_years=10, start=m0, nyear=nyear)[0]
            held(golden, (got, None), (want, None), table, 0, 'run_model {} {}'.format(var, kind))
            have = ~np.isnan(got[:, 1])
            assert have.sum() > w.ncell // 2 and (got[have, 1::2] <= got[have, 2::2]).all()
            # the interval holds the fit's own level in most cells (not all: the percentile interval is not centred on it)
            level = c.extremes[(var, kind)]['table'][:, 8:]
            inside = (got[have, 3::2] <= level[have]) & (level[have] <= got[have, 4::2])
            assert inside.mean() > 0.9
            lines = open(stem + '.csv').read().splitlines()
            assert lines[0] == 'id,nb,k_lo,k_hi,x_T2_lo,x_T2_hi,x_T10_lo,x_T10_hi,x_T100_lo,x_T100_hi' and len(lines) == w.ncell + 1
            text = np.array([[float(v or 'nan') for v in ln.split(',')] for ln in lines[1:]])   # (NaN is the empty field)
            assert (text[:, 0] == np.arange(1, w.ncell + 1)).all()                 # ids from 1
            assert np.array_equal(text[:, 1:], got, equal_nan=True)                # the csv parses back to the npy exactly
