"""GPU tests (-m gpu) of the standardized drought indices: xh_std_index through the C-ABI on the golden inputs (bound, NaN
masks, clipping, determinism, scales together against one by one, parameters out and in again, the fit against the
restatement's, the LDS size limit, the argument errors), run_model with [DroughtIndex] in every output format, in future mode
on a historic fit, and a three-member ensemble with statistics of the index.

The bound is sindex_cases.bound: 8 x the restatement's own error against the 40-digit golden, per input, distribution and
scale.  Measured on one MI355X (max |device - golden| over all elements; restatement in brackets):
    [70, 360]  gamma      k = 1: 1.82e-12 (1.82e-12)   3: 3.64e-12 (3.64e-12)   12: 5.2e-13 (5.24e-13)   24: 1.14e-12 (1.14e-12)
    [70, 72]   gamma      k = 1: 1.74e-12 (1.74e-12)   3: 1.6e-12 (1.6e-12)     12: 1.0e-12 (1.0e-12)    24: 1.79e-12 (1.79e-12)
    [70, 360]  empirical  every k: 2.2e-15 (2.0e-15)         [70, 72]  empirical  every k: <= 8.9e-16 (6.7e-16)
"""
import os
import re

import numpy as np
import pytest

import sindex_cases as cases
import sindex_np

pytestmark = pytest.mark.gpu


def same_bits(x, ref, tag=''):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, tag
    assert np.array_equal(x.view(np.uint64), ref.view(np.uint64)), '{}: {} values differ'.format(
        tag, int((x.view(np.uint64) != ref.view(np.uint64)).sum()))


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def run(ctx, x, scales, ref0, nyr, dist, par_in=None, want_par=False, max_shape=cases.MAX_SHAPE):
    """({k: index}, {k: parameters} or None) of one xh_std_index call; the outputs are pre-filled with a sentinel."""
    ncell, nmonths = x.shape
    d_x = ctx.upload(x)
    d_idx = [ctx.upload(np.full(x.shape, -7.0)) for _ in scales]
    d_out = [ctx.upload(np.full((ncell, 12, 4), -7.0)) for _ in scales] if want_par else None
    d_in = [ctx.upload(par_in[k]) for k in scales] if par_in is not None else None
    ctx.std_index(ncell, nmonths, scales, ref0, nyr, dist, max_shape, d_x, d_idx, par_in=d_in, par_out=d_out)
    idx = {k: a.download() for k, a in zip(scales, d_idx)}
    par = {k: a.download() for k, a in zip(scales, d_out)} if want_par else None
    for a in [d_x] + d_idx + (d_out or []) + (d_in or []):
        a.free()
    return idx, par


@pytest.mark.parametrize('dist', cases.DISTS)
@pytest.mark.parametrize('n', cases.INPUTS)
def test_index_on_the_golden_inputs(ctx, n, dist):
    x, ref0, nyr = cases.inputs(n)
    gamma = dist == 'gamma'
    together, par = run(ctx, x, cases.SCALES, ref0, nyr, dist, want_par=gamma)
    for k in cases.SCALES:
        cases.check_against_gold(together[k], n, dist, k, cases.bound(n, dist, k), 'device')
    # two calls: the same bits; one call per scale: the same bits as the scales together
    again, par2 = run(ctx, x, cases.SCALES, ref0, nyr, dist, want_par=gamma)
    for k in cases.SCALES:
        same_bits(again[k], together[k], 'second call, scale {}'.format(k))
        alone, _ = run(ctx, x, (k,), ref0, nyr, dist)
        same_bits(alone[k], together[k], 'scale {} alone'.format(k))
    if not gamma:
        return
    for k in cases.SCALES:
        same_bits(par2[k], par[k], 'parameters of the second call, scale {}'.format(k))
        # against the restatement's fit: the same NaN rows, q0 and n exact, alpha and beta to the cancellation in A
        ref = cases.restated(n, dist, k)[1]
        nan_rows = np.isnan(ref).any(-1)
        assert np.array_equal(np.isnan(par[k]), np.repeat(nan_rows[..., None], 4, -1)), k
        assert nan_rows.any() and not nan_rows.all()
        ok = ~nan_rows
        assert np.array_equal(par[k][ok][:, 0], ref[ok][:, 0]) and np.array_equal(par[k][ok][:, 3], ref[ok][:, 3])
        assert np.allclose(par[k][ok][:, 1:3], ref[ok][:, 1:3], rtol=1e-9, atol=0)
    # the fit handed back in: nothing is fitted, the index has the same bits
    fed, _ = run(ctx, x, cases.SCALES, ref0, nyr, dist, par_in=par)
    for k in cases.SCALES:
        same_bits(fed[k], together[k], 'par_out fed as par_in, scale {}'.format(k))
    # ... and on other data it is the table that counts: the 3-month table on the 1-month series is not the 1-month index
    other, _ = run(ctx, x, (1,), ref0, nyr, dist, par_in={1: par[3]})
    want = sindex_np.index_gamma(sindex_np.accumulate(x, 1), par[3])
    assert np.array_equal(np.isnan(other[1]), np.isnan(want))
    m = ~np.isnan(want)
    assert np.abs(other[1][m] - want[m]).max() <= cases.bound(n, dist, 1)


def test_the_longest_series_and_the_longest_scale(ctx):
    """4096 months (the limit: 64 KB + 384 B of LDS) at scales 1 and 48, three cells.  No golden at this size: held to the
    restatement within 1e-10 -- the shapes here are below 10, where A = log(mu) - ml loses ~ eps log(mu) / A ~ 1e-15 relative
    and both float64 implementations stay below 1e-13 of the exact index; 1e-10 says 'the same function' with room, and what
    the case is about (a launch at the LDS limit, a 48-term sum, 16 strides of the workgroup) fails by far more."""
    rng = np.random.default_rng(4096)
    for nm in (4096 // 12 * 12,):
        x = rng.gamma(2.0, 5.0, (3, nm)) * (1.0 + 0.5 * np.sin(2 * np.pi * np.arange(nm) / 12.0))
        x[1, rng.random(nm) < 0.2] = 0.0
        for dist in cases.DISTS:
            got, _ = run(ctx, x, (1, 48), 120, 300, dist)
            for k in (1, 48):
                want = sindex_np.std_index(x, k, 120, 300, dist)[0]
                assert np.array_equal(np.isnan(got[k]), np.isnan(want)), (dist, k)
                m = ~np.isnan(want)
                assert m.sum() >= 3 * (nm - 47) and np.abs(got[k][m] - want[m]).max() <= 1e-10, (dist, k)


def test_argument_errors_launch_nothing(ctx):
    from xanthos_amd import _hip
    x = np.ones((2, 24))
    d_x, d_i, d_p = ctx.upload(x), ctx.upload(np.full((2, 24), -7.0)), ctx.upload(np.full((2, 12, 4), -7.0))

    def refused(code, pattern, nmonths=24, scales=(1,), ref0=0, nyr=2, dist='gamma', max_shape=1000.0, x=d_x, index=(d_i,),
                par_in=None):
        with pytest.raises(_hip.HipError) as exc:
            ctx.std_index(2, nmonths, scales, ref0, nyr, dist, max_shape, x, list(index) * (len(scales) if len(index) == 1 else 1),
                          par_in=par_in)
        assert 'error {}'.format(code) in str(exc.value) and re.search(pattern, str(exc.value)), str(exc.value)
    refused(1, 'NULL', x=None)
    refused(1, 'index array of scale 0 is NULL', index=(None,))
    refused(1, 'par_in of scale 0 is NULL', par_in=[None])
    refused(1, 'whole years', nmonths=25)
    refused(3, '4096', nmonths=4104)
    refused(1, 'reference period', ref0=12, nyr=2)
    refused(1, 'reference period', ref0=6, nyr=1)
    refused(1, 'reference period', nyr=0)
    refused(3, 'outside 1..48', scales=(0,))
    refused(3, 'outside 1..48', scales=(1, 49))
    refused(3, 'nscale', scales=(1,) * 9)
    refused(1, 'empirical', dist='empirical', par_in=[d_p])
    refused(1, 'max_shape', max_shape=0.0)
    refused(1, 'max_shape', max_shape=float('nan'))
    with pytest.raises(_hip.HipError, match='nscale|NULL'):
        ctx.std_index(2, 24, (), 0, 2, 'gamma', 1000.0, d_x, [])
    ctx.sync()
    assert (d_i.download() == -7.0).all() and (d_p.download() == -7.0).all()
    ms, calls = ctx.timing('std_index')
    before = calls
    ctx.std_index(2, 24, (1,), 0, 2, 'gamma', 1000.0, d_x, [d_i])
    ctx.sync()
    assert ctx.timing('std_index')[1] == before + 1          # the timer's name


# ------------------------------------------------------------------ run_model and the ensemble
PROJECT = 'pm_abcd_mrtm_synth'
YEARS = (1971, 1976)
NPY, CSV = 4, 1
# Against the restatement on a run's own arrays there is no golden.  Both are float64 implementations of one definition: the
# restatement within E of the exact index, the device within 8 E, E the largest error measured for the restatement on the golden
# inputs -- whose rows reach the shape limit, where the error (the cancellation in A, ~ alpha) is largest.  So 9 E.
E2E_BOUND = {d: 9 * max(v for (n, dist, k), v in cases.MEASURED.items() if dist == d) for d in cases.DISTS}


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


def close_to_restatement(got, x, k, ref0, nyr, dist, par=None):
    want = sindex_np.std_index(x, k, ref0, nyr, dist, par=par)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (dist, k)
    m = ~np.isnan(want)
    assert m.mean() > 0.5
    err = float(np.abs(got[m] - want[m]).max())
    print('run_model {} k={}: max |index - restatement| {:.3g} (bound {:.3g})'.format(dist, k, err, E2E_BOUND[dist]))
    assert err <= E2E_BOUND[dist], (dist, k, err)


@pytest.fixture(scope='module')
def world():
    from xanthos_amd import synth
    w = synth.make_world(nrow=36, ncol=72, ncell=300, n_basins=3, seed=21)
    nm = 12 * (YEARS[1] - YEARS[0] + 1)
    return w, [synth.make_forcing(w, nm, seed=100 + 7 * k) for k in range(3)], nm


def example(root, world, drought_index=None, **kw):
    from xanthos_amd import synth
    w, forcings, nm = world
    kw.setdefault('output_vars', ('q', 'avgchflow', 'soilmoisture'))
    return synth.write_example(str(root), w, forcings[0], YEARS[0], YEARS[1], runoff_spinup=25, routing_spinup=6,
                               drought_index=drought_index, **kw)


def test_run_model_writes_the_index_and_nothing_else_changes(world, tmp_path):
    from xanthos_amd import run_model
    w, forcings, nm = world
    plain = run_model(example(tmp_path / 'plain', world, output_format=NPY, gridded=True))
    di = dict(index_var='q', scales=(1, 3, 12), reference_start_year=1972, reference_end_year=1976)
    c = run_model(example(tmp_path / 'index', world, output_format=NPY, gridded=True, drought_index=di))
    out_plain, out = [os.path.join(str(tmp_path), d, 'output', PROJECT) for d in ('plain', 'index')]
    same_files(out, out_plain, 'every other file', but=lambda rel: rel.startswith('drought_index_'))
    q = np.load(os.path.join(out, 'q_mmpermonth_{}.npy'.format(PROJECT)))
    assert sorted(c.drought_index) == [1, 3, 12] and sorted(c.drought_index_parameters) == [1, 3, 12]
    assert callable(plain.drought_index)                 # (without the flag the method has left nothing in its place)
    for k in (1, 3, 12):
        stem = os.path.join(out, 'drought_index_q_{}m_{}'.format(k, PROJECT))
        got = np.load(stem + '.npy')
        same_bits(got, c.drought_index[k], 'file and attribute')
        close_to_restatement(got, q, k, 12, 5, 'gamma')
        par = np.load(os.path.join(out, 'drought_index_q_{}m_parameters_{}.npy'.format(k, PROJECT)))
        assert par.shape == (w.ncell, 12, 4)
        same_bits(par, c.drought_index_parameters[k], 'parameter file')
        ok = ~np.isnan(par).any(-1)
        assert ok.mean() > 0.5 and (par[ok][:, 3] == 5).all()          # five reference years behind month k - 1
        assert os.path.getsize(stem + '_grid.nc') > 4 * nm * w.nrow * w.ncol
    # future mode on the historic fit: the same data indexed against the tables the run above wrote -> the same index bits
    fut = example(tmp_path / 'future', world, output_format=NPY, hist_flag=False, ch_storage=np.zeros(w.ncell),
                  drought_index=dict(di, parameters=os.path.join(out, PROJECT)))
    f = run_model(fut)
    out_f = os.path.join(str(tmp_path), 'future', 'output', PROJECT)
    assert f.drought_index_parameters is None
    assert not [n for n in os.listdir(out_f) if 'parameters' in n]
    for k in (1, 3, 12):
        same_bits(np.load(os.path.join(out_f, 'drought_index_q_{}m_{}.npy'.format(k, PROJECT))), c.drought_index[k], 'future')


@pytest.mark.parametrize('fmt, var, dist', [(CSV, 'avgchflow', 'empirical'), (0, 'soilmoisture', 'gamma'), (2, 'avgchflow', 'gamma')])
def test_run_model_in_every_output_format(world, tmp_path, fmt, var, dist):
    from xanthos_amd import run_model
    w, forcings, nm = world
    di = dict(index_var=var, scales=(3, 6), distribution=dist)
    c = run_model(example(tmp_path, world, output_format=fmt, drought_index=di))
    out = os.path.join(str(tmp_path), 'output', PROJECT)
    ext = {CSV: '.csv', 0: '.nc', 2: '.mat'}[fmt]
    src = {'avgchflow': c.Avg_ChFlow, 'soilmoisture': c.Sav}[var]
    for k in (3, 6):
        path = os.path.join(out, 'drought_index_{}_{}m_{}{}'.format(var, k, PROJECT, ext))
        assert os.path.getsize(path) > 4 * nm * w.ncell
        close_to_restatement(c.drought_index[k], src, k, 0, 6, dist)
        if fmt == CSV:                                    # shortest round-trip text: the file holds the same doubles
            head = open(path).readline().strip().split(',')
            assert head[:3] == ['id', '197101', '197102'] and len(head) == nm + 1
            same_bits(read_table(path), c.drought_index[k], 'csv')
            assert open(path).read().splitlines()[1].startswith('1,')
        assert os.path.isfile(os.path.join(out, 'drought_index_{}_{}m_parameters_{}.npy'.format(var, k, PROJECT))) == (dist == 'gamma')


def test_ensemble_members_and_statistics_of_the_index(world, tmp_path):
    import ens_np
    from xanthos_amd import Xanthos, run_model, synth
    w, forcings, nm = world
    stats = ('mean', 'q10')
    ini, members = synth.write_ensemble_example(str(tmp_path), w, forcings, YEARS[0], YEARS[1], runoff_spinup=25, routing_spinup=6,
                                                statistics=stats, statistics_vars=('q', 'index3'), output_format=NPY,
                                                drought_index=dict(index_var='q', scales=(1, 3)))
    res = run_model(ini)
    out = os.path.join(str(tmp_path), 'output', PROJECT)
    stack = []
    for member, overrides in members:
        ref = os.path.join(str(tmp_path), 'single', member)
        Xanthos(ini).execute(dict(overrides, OutputFolder=ref))
        same_files(os.path.join(out, member), ref, member)
        assert os.path.isfile(os.path.join(ref, 'drought_index_q_1m_{}.npy'.format(PROJECT)))
        stack.append(np.load(os.path.join(out, member, 'drought_index_q_3m_{}.npy'.format(PROJECT))))
    stack = np.stack(stack)
    assert sorted(res.statistics) == ['index3', 'q']
    for stat in stats:
        want = ens_np.numpy_stat(stack, stat)
        got = np.load(os.path.join(out, 'ensemble', 'drought_index_q_3m_{}_{}.npy'.format(PROJECT, stat)))
        assert 0 < np.isnan(want).mean() < 0.5
        same_bits(got, want, ('index3', stat, 'file'))
        same_bits(res.statistics['index3'][stat], want, ('index3', stat, 'result'))
    assert not [n for n in os.listdir(os.path.join(out, 'ensemble')) if '_1m_' in n]
    # member_outputs = 0: the same statistics, no member folders
    from xanthos_amd import run_ensemble
    res0 = run_ensemble(ini, member_outputs=0)
    for stat in stats:
        same_bits(res0.statistics['index3'][stat], ens_np.numpy_stat(stack, stat), ('index3', stat, 'member_outputs = 0'))
