"""GPU tests (-m gpu) of SPI / SPEI and the log-logistic distribution: xh_std_index2 through the C-ABI on the
golden inputs (bound, NaN masks, clipping, determinism, scales together against one by one, parameters out and in again, a
table of another scale), the subtrahend load against a host-subtracted array for all three distributions, the longest
series (the third LDS row near its limit), the argument errors, run_model with index_var = precip / balance, in future mode on
the first run's tables, and a two-member ensemble with statistics of the index.

The bound is spei_cases': 8 x the restatement's own error against the 40-digit golden per input and scale (met on the row
shifted by 1e6), and 8 x its error on the other rows for those.  Measured on one MI355X (max |device - golden|, all rows / the
rows but the shifted one; the restatement's figures are spei_cases.MEASURED / MEASURED_REST, the table is in DESIGN 4.19):
    [57, 360]  k = 1: 9.98e-09 / 9.15e-14   3: 6.73e-09 / 1.52e-13   12: 1.59e-09 / 1.56e-13   24: 2.46e-09 / 2.68e-13
    [57, 72]   k = 1: 5.62e-10 / 6.35e-14   3: 1.05e-09 / 6.49e-14   12: 2.33e-09 / 8.77e-14   24: 1.41e-10 / 5.77e-15
the same as the host build of the header to three digits.  4092 months: 9.3e-15 (scale 1) and 1.1e-14 (scale 48, |beta| up
to 996) from the restatement; run_model: 4.4e-15 (SPEI), 4.3e-14 (SPI, gamma).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import sindex_cases
import sindex_np
import spei_cases as cases
import spei_np

pytestmark = pytest.mark.gpu
LL = 'loglogistic'


def same_bits(x, ref, tag=''):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, tag
    assert np.array_equal(x.view(np.uint64), ref.view(np.uint64)), '{}: {} values differ'.format(
        tag, int((x.view(np.uint64) != ref.view(np.uint64)).sum()))


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def run(ctx, x, scales, ref0, nyr, dist=LL, par_in=None, want_par=False, minus=None, max_shape=cases.MAX_SHAPE):
    """({k: index}, {k: parameters} or None) of one xh_std_index2 call; the outputs are pre-filled with a sentinel."""
    ncell, nmonths = x.shape
    d_x = ctx.upload(np.ascontiguousarray(x, dtype=np.float64))
    d_m = ctx.upload(np.ascontiguousarray(minus, dtype=np.float64)) if minus is not None else None
    d_idx = [ctx.upload(np.full(x.shape, -7.0)) for _ in scales]
    d_out = [ctx.upload(np.full((ncell, 12, 4), -7.0)) for _ in scales] if want_par else None
    d_in = [ctx.upload(par_in[k]) for k in scales] if par_in is not None else None
    ctx.std_index(ncell, nmonths, scales, ref0, nyr, dist, max_shape, d_x, d_idx, par_in=d_in, par_out=d_out, minus=d_m)
    idx = {k: a.download() for k, a in zip(scales, d_idx)}
    par = {k: a.download() for k, a in zip(scales, d_out)} if want_par else None
    for a in [d_x] + ([d_m] if d_m is not None else []) + d_idx + (d_out or []) + (d_in or []):
        a.free()
    return idx, par


@pytest.mark.parametrize('n', cases.INPUTS)
def test_index_on_the_golden_inputs(ctx, n):
    x, ref0, nyr = cases.inputs(n)
    together, par = run(ctx, x, cases.SCALES, ref0, nyr, want_par=True)
    for k in cases.SCALES:
        cases.check_against_gold(together[k], n, k, cases.FACTOR, 'device')
        cases.check_parameters(par[k], n, k, 'device')
        ref = cases.restated(n, k)[1]                      # the restatement's fit: the same sums in the same order
        ok = ~np.isnan(ref).any(-1)
        assert np.allclose(par[k][ok], ref[ok], rtol=1e-12, atol=0), k
    # two calls: the same bits; one call per scale: the same bits as the scales together
    again, par2 = run(ctx, x, cases.SCALES, ref0, nyr, want_par=True)
    for k in cases.SCALES:
        same_bits(again[k], together[k], 'second call, scale {}'.format(k))
        same_bits(par2[k], par[k], 'parameters of the second call, scale {}'.format(k))
        alone, par_alone = run(ctx, x, (k,), ref0, nyr, want_par=True)
        same_bits(alone[k], together[k], 'scale {} alone'.format(k))
        same_bits(par_alone[k], par[k], 'parameters of scale {} alone'.format(k))
    # the fit handed back in: nothing is ranked or fitted, the index has the same bits
    fed, _ = run(ctx, x, cases.SCALES, ref0, nyr, par_in=par)
    for k in cases.SCALES:
        same_bits(fed[k], together[k], 'par_out fed as par_in, scale {}'.format(k))
    # ... and on other data it is the table that counts: the 3-month table on the 1-month series
    other, _ = run(ctx, x, (1,), ref0, nyr, par_in={1: par[3]})
    want = spei_np.index(sindex_np.accumulate(x, 1), par[3])
    assert np.array_equal(np.isnan(other[1]), np.isnan(want))
    m = ~np.isnan(want)
    assert not np.array_equal(other[1][m], together[1][m])
    assert np.abs(other[1][m] - want[m]).max() <= cases.bound(n, 1)


@pytest.mark.parametrize('dist', ('gamma', 'empirical', LL))
def test_subtrahend_equals_the_host_subtracted_array(ctx, dist):
    """xh_std_index2 with d_minus against xh_std_index (the 13-argument entry, called as such) on a - b formed by numpy: one
    rounded subtraction either way, so the same bits.  The minuend and the subtrahend are both inexact in their difference
    (a = x + y rounded), and for gamma / empirical the difference keeps the zeros and the negative value of the 4.18 input."""
    from xanthos_amd import _hip
    x, ref0, nyr = cases.inputs(360) if dist == LL else sindex_cases.inputs(360)
    x = x * 1.0000001                                      # (the golden inputs are float32 values: (x + b) - b would be x)
    rng = np.random.default_rng(11)
    b = rng.gamma(2.0, 3.0, x.shape)
    a = x + b
    zero = x == 0
    a[zero] = b[zero]                                      # (the zeros stay zeros)
    d = a - b
    assert (d != x).mean() > 0.3 and (np.isnan(d) == np.isnan(x)).all() and (d[zero] == 0).all()
    scales = (1, 3, 12)
    got, gpar = run(ctx, a, scales, ref0, nyr, dist, minus=b, want_par=dist != 'empirical')
    # the reference: the old entry, straight through ctypes
    ncell, nmonths = d.shape
    d_d = ctx.upload(d)
    d_idx = [ctx.upload(np.full(d.shape, -7.0)) for _ in scales]
    d_par = [ctx.upload(np.full((ncell, 12, 4), -7.0)) for _ in scales]
    k = np.array(scales, dtype=np.int32)
    table = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ptr for a in arrs])
    rc = _hip.lib().xh_std_index(ctx.handle, ncell, nmonths, len(scales), k.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ref0, nyr,
                                 _hip.STD_INDEX_DIST2[dist], cases.MAX_SHAPE, d_d.ptr, None, table(d_par), table(d_idx))
    assert rc == 0
    for i, s in enumerate(scales):
        want = d_idx[i].download()
        assert not (want == -7.0).any() and (~np.isnan(want)).mean() > 0.5
        same_bits(got[s], want, '{} scale {}'.format(dist, s))
        if gpar is not None:
            same_bits(gpar[s], d_par[i].download(), '{} parameters, scale {}'.format(dist, s))
    for arr in [d_d] + d_idx + d_par:
        arr.free()


def test_the_longest_series_and_the_longest_scale(ctx):
    """4092 months with a 300-year reference period: n = 300 per calendar month, 3600 elements to rank, the third LDS row and
    98,592 B of LDS, near the limit; scales 1 and 48 on 100 cells.  No golden at this size: held to the restatement within
    1e-10 -- both form the same sums in the same order, so beta has the same bits and alpha and gamma differ by the last bits
    of sin alone; exp(beta log z) moves by |beta| <= 1000 times an ulp of log, below 1e-12; 1e-10 says 'the same function'
    with room, and what the case is about (a launch at the LDS limit, ranks among 300, 16 strides of the
    workgroup) fails by far more."""
    rng = np.random.default_rng(4092)
    nm, ncell = 4092, 100
    x = rng.gamma(2.0, 5.0, (ncell, nm)) * (1.0 + 0.5 * np.sin(2 * np.pi * np.arange(nm) / 12.0)) - 9.0
    x[1] = np.round(x[1])                                  # ties
    x[2, 777] = np.nan
    got, par = run(ctx, x, (1, 48), 120, 300, want_par=True)
    for k in (1, 48):
        want, want_par = spei_np.std_index(x, k, 120, 300)
        assert (par[k][0, :, 3] == 300).all()
        assert np.array_equal(np.isnan(par[k]), np.isnan(want_par)), k
        assert np.array_equal(np.isnan(got[k]), np.isnan(want)), k
        m = ~np.isnan(want)
        err = float(np.abs(got[k][m] - want[m]).max())
        print('4092 months, scale {}: max |device - restatement| {:.3g}, max |beta| {:.3g}'.format(k, err, np.nanmax(np.abs(want_par[..., 1]))))
        assert m.mean() > 0.9 and err <= 1e-10, (k, err)
    assert np.isnan(got[1][2, 777 % 12::12]).all() and not np.isnan(got[1][2, (777 + 1) % 12::12]).any()


def test_argument_errors_launch_nothing(ctx):
    from xanthos_amd import _hip
    x = np.ones((2, 24))
    d_x, d_i, d_p = ctx.upload(x), ctx.upload(np.full((2, 24), -7.0)), ctx.upload(np.full((2, 12, 4), -7.0))
    k = np.array([1], dtype=np.int32)
    kp = k.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    one = lambda a: (ctypes.c_void_p * 1)(a.ptr if a is not None else None)

    def refused(code, pattern, rc):
        assert rc == code
        with pytest.raises(_hip.HipError) as exc:
            ctx._check(rc)
        assert 'error {}'.format(code) in str(exc.value) and re.search(pattern, str(exc.value)), str(exc.value)
    lib = _hip.lib()
    for entry, extra in ((lib.xh_std_index2, (None,)), (lib.xh_std_index, ())):
        refused(1, r'dist \(3\)', entry(ctx.handle, 2, 24, 1, kp, 0, 2, 3, 1000.0, d_x.ptr, *extra, None, one(d_p), one(d_i)))
        refused(1, r'dist \(-1\)', entry(ctx.handle, 2, 24, 1, kp, 0, 2, -1, 1000.0, d_x.ptr, *extra, None, one(d_p), one(d_i)))
    refused(1, 'index array of scale 0 is NULL', lib.xh_std_index2(ctx.handle, 2, 24, 1, kp, 0, 2, 2, 1000.0, d_x.ptr, d_x.ptr, None,
                                                                   one(d_p), one(None)))
    refused(1, 'NULL', lib.xh_std_index2(ctx.handle, 2, 24, 1, kp, 0, 2, 2, 1000.0, d_x.ptr, None, None, one(d_p), None))
    refused(1, 'NULL', lib.xh_std_index2(ctx.handle, 2, 24, 1, kp, 0, 2, 2, 1000.0, None, d_x.ptr, None, one(d_p), one(d_i)))
    refused(1, 'par_in of scale 0 is NULL', lib.xh_std_index2(ctx.handle, 2, 24, 1, kp, 0, 2, 2, 1000.0, d_x.ptr, None, one(None),
                                                              one(d_p), one(d_i)))
    refused(1, 'empirical', lib.xh_std_index2(ctx.handle, 2, 24, 1, kp, 0, 2, 1, 1000.0, d_x.ptr, d_x.ptr, one(d_p), None, one(d_i)))
    refused(3, '4096', lib.xh_std_index2(ctx.handle, 2, 4104, 1, kp, 0, 2, 2, 1000.0, d_x.ptr, None, None, one(d_p), one(d_i)))
    refused(1, 'max_shape', lib.xh_std_index2(ctx.handle, 2, 24, 1, kp, 0, 2, 2, 0.0, d_x.ptr, None, None, one(d_p), one(d_i)))
    with pytest.raises(ValueError, match='loglogistic'):
        ctx.std_index(2, 24, (1,), 0, 2, 'weibull', 1000.0, d_x, [d_i])
    ctx.sync()
    assert (d_i.download() == -7.0).all() and (d_p.download() == -7.0).all()
    before = ctx.timing('std_index')[1]
    ctx.std_index(2, 24, (1,), 0, 2, LL, 1000.0, d_x, [d_i], par_out=[d_p], minus=d_x)
    ctx.sync()
    assert ctx.timing('std_index')[1] == before + 1          # the timer's name
    assert np.isnan(d_i.download()).all() and np.isnan(d_p.download()).all()      # (1 - 1: a constant sample)
    for a in (d_x, d_i, d_p):
        a.free()


# ------------------------------------------------------------------ run_model and the ensemble
PROJECT = 'pm_abcd_mrtm_synth'
YEARS = (1971, 1976)
NPY, CSV = 4, 1
# Against the restatement on a run's own arrays there is no golden.  Both are float64 implementations of one definition: the
# restatement within E of the exact index, the device within 8 E, E the largest error measured for the restatement on the golden
# inputs -- whose rows reach the worst conditioning a run can bring.  So 9 E (DESIGN 4.18's argument).
E2E_BOUND = {LL: 9 * max(cases.MEASURED.values()),
             'gamma': 9 * max(v for (n, dist, k), v in sindex_cases.MEASURED.items() if dist == 'gamma')}


def files_of(folder, skip=('logfile.log',)):
    out = {}
    for base, _, names in os.walk(folder):
        for f in names:
            if f not in skip:
                out[os.path.relpath(os.path.join(base, f), folder)] = os.path.join(base, f)
    return out


def same_files(a, b, tag='', but=lambda rel: False):
    import filecmp
    fa = {k: v for k, v in files_of(a).items() if not but(k)}
    fb = {k: v for k, v in files_of(b).items() if not but(k)}
    assert sorted(fa) == sorted(fb) and fa, (tag, sorted(fa), sorted(fb))
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), (tag, rel)


def read_table(path):
    if path.endswith('.npy'):
        return np.load(path)
    rows = open(path).read().splitlines()[1:]
    return np.array([[float(v) if v != '' else np.nan for v in r.split(',')[1:]] for r in rows])


def close_to_restatement(got, x, k, ref0, nyr, dist, minus=None):
    if dist == LL:
        want = spei_np.std_index(x, k, ref0, nyr, minus=minus)[0]
    else:
        want = sindex_np.std_index(x if minus is None else x - minus, k, ref0, nyr, dist)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (dist, k)
    m = ~np.isnan(want)
    assert m.mean() > 0.3
    err = float(np.abs(got[m] - want[m]).max())
    print('run_model {} k={}: max |index - restatement| {:.3g} (bound {:.3g}), {:.0%} of the elements'.format(
        dist, k, err, E2E_BOUND[dist], m.mean()))
    assert err <= E2E_BOUND[dist], (dist, k, err)


@pytest.fixture(scope='module')
def world():
    from xanthos_amd import synth
    w = synth.make_world(nrow=36, ncol=72, ncell=300, n_basins=3, seed=21)
    nm = 12 * (YEARS[1] - YEARS[0] + 1)
    return w, [synth.make_forcing(w, nm, seed=100 + 7 * k) for k in range(2)], nm


def example(root, world, drought_index=None, **kw):
    from xanthos_amd import synth
    w, forcings, nm = world
    kw.setdefault('output_vars', ('q', 'avgchflow', 'soilmoisture'))
    return synth.write_example(str(root), w, forcings[0], YEARS[0], YEARS[1], runoff_spinup=25, routing_spinup=6,
                               drought_index=drought_index, **kw)


def test_run_model_spei_and_nothing_else_changes(world, tmp_path):
    from xanthos_amd import run_model
    w, forcings, nm = world
    run_model(example(tmp_path / 'plain', world, output_format=NPY))
    di = dict(index_var='balance', scales=(1, 3, 12), distribution=LL)
    c = run_model(example(tmp_path / 'index', world, output_format=NPY, drought_index=di))
    out_plain, out = [os.path.join(str(tmp_path), d, 'output', PROJECT) for d in ('plain', 'index')]
    same_files(out, out_plain, 'every other file', but=lambda rel: rel.startswith('drought_index_'))
    precip, pet = c.pipe.forcing['precip'].download(), np.asarray(c.PET)
    assert precip.shape == pet.shape == (w.ncell, nm) and ((precip - pet) < 0).mean() > 0.1
    assert sorted(c.drought_index) == [1, 3, 12] and sorted(c.drought_index_parameters) == [1, 3, 12]
    for k in (1, 3, 12):
        got = np.load(os.path.join(out, 'drought_index_balance_{}m_{}.npy'.format(k, PROJECT)))
        same_bits(got, c.drought_index[k], 'file and attribute')
        close_to_restatement(got, precip, k, 0, 6, LL, minus=pet)
        par = np.load(os.path.join(out, 'drought_index_balance_{}m_llparameters_{}.npy'.format(k, PROJECT)))
        assert par.shape == (w.ncell, 12, 4)
        same_bits(par, c.drought_index_parameters[k], 'parameter file')
        ok = ~np.isnan(par).any(-1)
        assert ok.mean() > 0.3 and set(par[ok][:, 3]) <= {5.0, 6.0} and (np.abs(par[ok][:, 1]) > 1).all()
        assert not os.path.exists(os.path.join(out, 'drought_index_balance_{}m_parameters_{}.npy'.format(k, PROJECT)))
    # a second run indexed against the tables the first wrote: the same data, the same index bits, nothing fitted
    again = run_model(example(tmp_path / 'again', world, output_format=NPY, drought_index=dict(di, parameters=os.path.join(out, PROJECT))))
    out_a = os.path.join(str(tmp_path), 'again', 'output', PROJECT)
    assert again.drought_index_parameters is None
    assert not [n for n in os.listdir(out_a) if 'parameters' in n]
    for k in (1, 3, 12):
        same_bits(np.load(os.path.join(out_a, 'drought_index_balance_{}m_{}.npy'.format(k, PROJECT))), c.drought_index[k], 'second run')


def test_run_model_spi_with_gamma_in_csv(world, tmp_path):
    from xanthos_amd import run_model
    w, forcings, nm = world
    c = run_model(example(tmp_path, world, output_format=CSV, drought_index=dict(index_var='precip', scales=(3, 6), distribution='gamma')))
    out = os.path.join(str(tmp_path), 'output', PROJECT)
    precip = c.pipe.forcing['precip'].download()
    for k in (3, 6):
        path = os.path.join(out, 'drought_index_precip_{}m_{}.csv'.format(k, PROJECT))
        head = open(path).readline().strip().split(',')
        assert head[:3] == ['id', '197101', '197102'] and len(head) == nm + 1
        same_bits(read_table(path), c.drought_index[k], 'csv')
        close_to_restatement(c.drought_index[k], precip, k, 0, 6, 'gamma')
        assert os.path.isfile(os.path.join(out, 'drought_index_precip_{}m_parameters_{}.npy'.format(k, PROJECT)))
        assert not os.path.exists(os.path.join(out, 'drought_index_precip_{}m_llparameters_{}.npy'.format(k, PROJECT)))


def test_ensemble_member_with_its_own_precipitation(world, tmp_path):
    from xanthos_amd import run_ensemble
    w, forcings, nm = world
    ini = example(tmp_path, world, output_format=NPY, drought_index=dict(index_var='balance', scales=(1, 3), distribution=LL))
    wet = os.path.join(str(tmp_path), 'wet_precip.npy')
    np.save(wet, forcings[1]['precip'])
    res = run_ensemble(ini, members=[('base', {}), ('wet', {'PrecipitationFile': wet})], statistics=('mean',),
                       statistics_vars=('index3',))
    out = os.path.join(str(tmp_path), 'output', PROJECT)
    stack = np.stack([np.load(os.path.join(out, m, 'drought_index_balance_3m_{}.npy'.format(PROJECT))) for m in ('base', 'wet')])
    both = ~np.isnan(stack).any(0)
    assert both.mean() > 0.2 and (stack[0][both] != stack[1][both]).mean() > 0.9      # the members' SPEI differ
    for m in ('base', 'wet'):
        assert os.path.isfile(os.path.join(out, m, 'drought_index_balance_1m_llparameters_{}.npy'.format(PROJECT)))
    with np.errstate(all='ignore'):
        want = np.mean(stack, axis=0)
    got = np.load(os.path.join(out, 'ensemble', 'drought_index_balance_3m_{}_mean.npy'.format(PROJECT)))
    same_bits(got, want, 'index3 mean, file')
    same_bits(res.statistics['index3']['mean'], want, 'index3 mean, result')
    assert sorted(res.statistics) == ['index3']
    assert not [n for n in os.listdir(os.path.join(out, 'ensemble')) if '_1m_' in n]


def test_spi_of_a_run_that_goes_stage_by_stage(world, tmp_path):
    """PET from a file (pet_module = none) with ABCD runs stage by stage on host arrays: no pipeline holds the forcing, and
    SPI indexes the loader's ``data.precip``."""
    from xanthos_amd import run_model
    w, forcings, nm = world
    ini = example(tmp_path, world, output_format=NPY, drought_index=dict(index_var='precip', scales=(3,), distribution='gamma'))
    pet_file = os.path.join(str(tmp_path), 'pet.npy')
    np.save(pet_file, np.full((w.ncell, nm), 60.0))
    text, n = re.subn(r'(?s)\[PET\].*?\n\[Runoff\]', '[PET]\npet_module = none\npet_file = {}\n\n[Runoff]'.format(pet_file), open(ini).read())
    assert n == 1
    open(ini, 'w').write(text)
    c = run_model(ini)
    assert c.pipe is None
    got = np.load(os.path.join(str(tmp_path), 'output', PROJECT, 'drought_index_precip_3m_{}.npy'.format(PROJECT)))
    same_bits(got, c.drought_index[3], 'file and attribute')
    close_to_restatement(got, np.asarray(c.data.precip, dtype=np.float64), 3, 0, 6, 'gamma')
