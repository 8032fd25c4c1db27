"""GPU tests (-m gpu) of the parameter ensemble: xh_basin_kge through the C-ABI against numpy (skill_np), and run_ensemble()
with abcd_pars members on small synthetic worlds -- members byte-identical to single runs with calib_file set to the same
table, the overlapped schedule equal to the serial one, the statistics equal to numpy, one upload and one PET for a
resident ensemble (S of each for a mixed one), and each member's KGE against observed basin runoff."""
import filecmp
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

import ens_np
import skill_np

pytestmark = pytest.mark.gpu


def same_bits(x, ref, tag=''):
    x, ref = np.asarray(x), np.asarray(ref)
    assert x.shape == ref.shape, tag
    assert np.array_equal(np.isnan(x), np.isnan(ref)), 'NaN masks differ ' + str(tag)
    m = ~np.isnan(ref)
    assert np.array_equal(x[m], ref[m]), '{}: {} of {} values differ'.format(tag, int((x[m] != ref[m]).sum()), int(m.sum()))


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


# ------------------------------------------------------------------ 1. the kernel through the C-ABI
NCELL = 500
SIZES = (1, 63, 64, 65, 300, 7)          # cells per basin: one, a wave less one, a wave, a wave and one, many, a few
ALL_NAN, NAN_MONTH = 5, 1                # the basin whose Q is NaN everywhere; the basin that is NaN in one whole month


def kernel_case(nmonths):
    """Interleaved membership (a shuffle), Q >= 0 with NaNs, areas, and observations = the numpy series x a smooth
    perturbation."""
    rng = np.random.default_rng(1000 + nmonths)
    label = rng.permutation(np.repeat(np.arange(len(SIZES)), SIZES))
    cells = [np.flatnonzero(label == b) for b in range(len(SIZES))]
    assert [len(c) for c in cells] == list(SIZES) and any(np.any(np.diff(c) > 1) for c in cells)
    q = rng.gamma(2.0, 15.0, size=(NCELL, nmonths))
    q[cells[4][[3, 120, 250]], [0, nmonths // 2, nmonths - 1]] = np.nan         # three scattered
    q[cells[ALL_NAN]] = np.nan
    q[cells[NAN_MONTH], 5] = np.nan
    area = rng.uniform(500.0, 3000.0, size=NCELL)
    return cells, q, area


def observations_for(series):
    m = np.arange(series.shape[1])
    return np.stack([s * (1.15 + 0.25 * np.sin(2 * np.pi * m / 12.0 + j)) for j, s in enumerate(series)])


@pytest.mark.parametrize('unit', ['km3_per_mth', 'mm_per_mth'])
@pytest.mark.parametrize('nmonths', [36, 130])       # below one wave; three waves of months, the last a tail of 2
def test_basin_kge_equals_numpy(ctx, nmonths, unit):
    cells, q, area = kernel_case(nmonths)
    nb = len(cells)
    ref_series, _ = skill_np.skill(q, area, cells, np.ones((nb, nmonths)), unit)
    obs = observations_for(ref_series)
    ref_series, ref_ed = skill_np.skill(q, area, cells, obs, unit)
    finite = ~np.isnan(ref_ed)
    assert list(np.flatnonzero(~finite)) == [ALL_NAN]                       # (its series is all zeros: 0 / 0)
    assert np.all((ref_ed[finite] >= 0.01) & (ref_ed[finite] <= 2.0)), ref_ed
    assert not np.isnan(ref_series).any() and np.all(ref_series[NAN_MONTH, 5] == 0.0)
    start = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    d = SimpleNamespace(start=ctx.upload(start, dtype=np.int64), cells=ctx.upload(np.concatenate(cells), dtype=np.int32),
                        q=ctx.upload(q), area=ctx.upload(area) if unit == 'km3_per_mth' else None, obs=ctx.upload(obs),
                        series=ctx.empty((nb, nmonths)), ed=ctx.empty((nb,)))

    def call(series):
        d.ed.upload(np.full(nb, -1.0))
        ctx.basin_kge(NCELL, nmonths, nb, d.start, d.cells, d.q, d.area, d.obs, d.ed, series=series)
        return d.ed.download()
    ed = call(d.series)
    series = d.series.download()
    print('series: max rel err {:.3e}; ED: max rel err {:.3e}'.format(
        float(np.max(np.abs(series - ref_series) / np.maximum(np.abs(ref_series), 1e-300))),
        float(np.max(np.abs(ed[finite] - ref_ed[finite]) / ref_ed[finite]))))
    assert np.array_equal(np.isnan(series), np.isnan(ref_series))
    assert np.all(np.abs(series - ref_series) <= 1e-12 * np.abs(ref_series))
    assert np.array_equal(np.isnan(ed), np.isnan(ref_ed)), (ed, ref_ed)
    assert np.all(np.abs(ed[finite] - ref_ed[finite]) <= 1e-9 * np.abs(ref_ed[finite])), (ed, ref_ed)
    d.series.upload(np.zeros((nb, nmonths)))
    same_bits(call(d.series), ed, 'second call')
    same_bits(d.series.download(), series, 'second call, series')
    same_bits(call(None), ed, 'without the series output')
    for a in vars(d).values():
        if a is not None:
            a.free()


def test_basin_kge_arguments(ctx):
    from xanthos_amd import _hip
    one, obs, ed = ctx.upload(np.ones(8)), ctx.upload(np.arange(4.0)), ctx.upload(np.zeros(1))
    start, cells = ctx.upload(np.array([0, 2]), dtype=np.int64), ctx.upload(np.array([0, 1]), dtype=np.int32)
    good = dict(ncell=2, nmonths=4, nbasins=1, start=start, cells=cells, q=one, area=None, obs=obs, ed=ed)
    for bad in (dict(q=None), dict(nbasins=0), dict(nbasins=-1), dict(nmonths=1), dict(obs=None), dict(ed=None),
                dict(start=None), dict(cells=None), dict(ncell=0)):
        with pytest.raises(_hip.HipError, match='error {}'.format(_hip.XH_ERR_ARG)):
            ctx.basin_kge(**dict(good, **bad))
    ctx.basin_kge(**good)                                  # (a constant series: NaN, as numpy)
    assert np.isnan(ed.download()[0])
    for a in (one, obs, ed, start, cells):
        a.free()


# ------------------------------------------------------------------ the driver on small synthetic worlds
NM, YEARS = 36, (1971, 1973)
STATS = ('mean', 'std', 'q50')
STAT_VARS = ('q', 'avgchflow')
LB = 1e-4
BOX_LO, BOX_HI = np.full(5, LB), np.array([1 - LB, 8 - LB, 1 - LB, 1 - LB, 1 - LB])      # the calibration's box of a, b, c, d, m


def files_of(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            if n != 'logfile.log':
                out[os.path.relpath(os.path.join(base, n), folder)] = os.path.join(base, n)
    return out


def same_files(a, b, tag=''):
    fa, fb = files_of(a), files_of(b)
    assert sorted(fa) == sorted(fb) and fa, (tag, sorted(fa), sorted(fb))
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), (tag, rel)


def read_table(path):
    if path.endswith('.npy'):
        return np.load(path)
    rows = open(path).read().splitlines()[1:]
    return np.array([[float(v) if v != '' else np.nan for v in r.split(',')[1:]] for r in rows])


class Counters:
    """DevicePipeline.set_forcing / run_pet wrapped with counters for the length of a ``with`` block."""

    def __enter__(self):
        from xanthos_amd.pipeline import DevicePipeline
        self.cls, self.calls = DevicePipeline, {'set_forcing': 0, 'run_pet': 0}
        self.kept = {name: getattr(DevicePipeline, name) for name in self.calls}
        for name, fn in self.kept.items():
            setattr(DevicePipeline, name, self.wrap(name, fn))
        return self

    def wrap(self, name, fn):
        def counted(pipe, *a, **kw):
            self.calls[name] += 1
            return fn(pipe, *a, **kw)
        return counted

    def __exit__(self, *exc):
        for name, fn in self.kept.items():
            setattr(self.cls, name, fn)


@pytest.fixture(scope='module', params=['pm', 'hargreaves'])
def runs(request, tmp_path_factory):
    """One world per configuration: the single runs of three parameter tables (and of one with another precipitation), the
    observations made from the first, and the resident ensemble overlapped and serial.  Computed once, read by the tests."""
    from xanthos_amd import Xanthos, run_ensemble, synth
    root = str(tmp_path_factory.mktemp('pens_' + request.param))
    w = synth.make_world(nrow=36, ncol=72, ncell=300, n_basins=3, seed=21)
    f, f2 = synth.make_forcing(w, NM, seed=61), synth.make_forcing(w, NM, seed=62)
    if request.param == 'pm':
        project, ext = 'pm_abcd_mrtm_synth', 'npy'
        ini = synth.write_example(root, w, f, *YEARS, runoff_spinup=25, routing_spinup=6, output_format=4)
    else:
        project, ext = 'hargreaves_abcd_mrtm_synth', 'csv'
        ini = synth.write_hgm_example(root, w, synth.hgm_forcing(w, f), *YEARS, project=project, runoff='abcd', runoff_spinup=25)
    out = os.path.join(root, 'output', project)
    lo = np.clip(w.abcd_pars * np.array([0.9, 1.1, 0.85, 1.2, 0.95]), BOX_LO, BOX_HI)
    hi = np.clip(w.abcd_pars * np.array([1.05, 0.9, 1.1, 0.8, 1.1]), BOX_LO, BOX_HI)
    assert not np.array_equal(lo, w.abcd_pars) and not np.array_equal(hi, w.abcd_pars)
    lo_file = os.path.join(root, 'pars_lo.npy')
    np.save(lo_file, lo)
    wet_file = os.path.join(root, 'pr_wet.npy')
    np.save(wet_file, f2['precip'])
    members = [('own', {}), ('lo', {'abcd_pars': lo_file}), ('hi', {'abcd_pars': hi})]
    mixed = members[:2] + [('wet', {'abcd_pars': hi, 'PrecipitationFile': wet_file})]
    single = {}
    for name, overrides in members + mixed[2:]:
        single[name] = os.path.join(root, 'single', name)
        args = {('calib_file' if k == 'abcd_pars' else k): v for k, v in overrides.items()}
        Xanthos(ini).execute(dict(args, OutputFolder=single[name]))
    q_file = 'q_mmpermonth_{}.{}'.format(project, ext)
    basins = sorted(set(int(b) for b in w.basin_ids))
    cells = skill_np.cells_of(w.basin_ids, basins)
    q_own = read_table(os.path.join(single['own'], q_file))
    series, _ = skill_np.skill(q_own, w.area, cells, np.ones((len(basins), NM)))
    obs = observations_for(series)
    obs_rows = np.array([[b, 0.0, 0.0, v] for b, row in zip(basins, obs) for v in row])
    kw = dict(members=members, statistics=STATS, statistics_vars=STAT_VARS, observed=obs_rows, obs_unit='km3_per_mth')
    with Counters() as counted:
        overlapped = run_ensemble(ini, overlap=True, **kw)
    kept = out + '_overlapped'
    os.rename(out, kept)
    serial = run_ensemble(ini, overlap=False, **kw)
    return SimpleNamespace(root=root, world=w, ini=ini, out=out, project=project, ext=ext, members=members, mixed=mixed,
                           single=single, q_file=q_file, basins=basins, cells=cells, obs=obs, obs_rows=obs_rows,
                           overlapped=overlapped, overlapped_out=kept, serial=serial, calls=dict(counted.calls))


# ---- 2. members equal single runs
def test_members_equal_single_runs_with_calib_file(runs):
    res = runs.overlapped
    assert res.names == ['own', 'lo', 'hi'] and [os.path.basename(d) for d in res.member_dirs] == res.names
    for name in res.names:
        same_files(os.path.join(runs.overlapped_out, name), runs.single[name], name)
    tables = [read_table(os.path.join(runs.single[n], runs.q_file)) for n in res.names]
    assert not np.array_equal(tables[0], tables[1], equal_nan=True) and not np.array_equal(tables[1], tables[2], equal_nan=True)
    assert sorted(os.listdir(runs.overlapped_out)) == sorted(['ensemble', 'logfile.log'] + res.names)


def test_statistics_equal_numpy_over_the_member_files(runs):
    for var in STAT_VARS:
        unit = 'm3persec' if var == 'avgchflow' else 'mmpermonth'
        stack = np.stack([read_table(os.path.join(runs.single[n], '{}_{}_{}.{}'.format(var, unit, runs.project, runs.ext)))
                          for n in runs.overlapped.names])
        for stat in STATS:
            got = read_table(os.path.join(runs.overlapped_out, 'ensemble',
                                          '{}_{}_{}_{}.{}'.format(var, unit, runs.project, stat, runs.ext)))
            ref = ens_np.numpy_stat(stack, stat)
            same_bits(got, ref, (var, stat, 'file'))
            same_bits(got, ens_np.stat(stack, stat), (var, stat, 'ens_np'))
            same_bits(runs.overlapped.statistics[var][stat], ref, (var, stat, 'result'))
            assert np.isnan(ref).mean() < 0.05


def test_overlap_changes_no_bit(runs):
    same_files(runs.overlapped_out, runs.out, 'overlap')                     # the whole tree: members, statistics, member_kge.csv
    for var in STAT_VARS:
        for stat in STATS:
            same_bits(runs.serial.statistics[var][stat], runs.overlapped.statistics[var][stat], (var, stat))
    same_bits(runs.serial.kge, runs.overlapped.kge, 'kge')


# ---- 3. resident state
def test_resident_ensemble_uploads_once_and_runs_pet_once(runs):
    assert runs.calls == {'set_forcing': 1, 'run_pet': 1}
    res = runs.overlapped
    assert len(res.forcing_upload[0]) > 0 and res.forcing_upload[1:] == [{}, {}]
    assert res.timings['upload'][0] > 0.0 and res.timings['upload'][1:] == [0.0, 0.0]


def test_mixed_ensemble_uploads_per_member_and_equals_single_runs(runs):
    from xanthos_amd import run_ensemble
    moved = runs.out + '_serial'
    os.rename(runs.out, moved)
    try:
        with Counters() as counted:
            res = run_ensemble(runs.ini, members=runs.mixed)
        assert counted.calls == {'set_forcing': 3, 'run_pet': 3}
        assert all(len(u) > 0 for u in res.forcing_upload) and res.kge is None and res.kge_basins is None
        for name in res.names:
            same_files(os.path.join(runs.out, name), runs.single[name], name)
        wet, hi = (read_table(os.path.join(runs.single[n], runs.q_file)) for n in ('wet', 'hi'))
        assert not np.array_equal(wet, hi, equal_nan=True)
        assert sorted(os.listdir(runs.out)) == sorted(['logfile.log'] + res.names)
    finally:
        shutil.rmtree(runs.out, ignore_errors=True)
        os.rename(moved, runs.out)


# ---- 4. skill through the driver
def test_member_kge_equals_numpy_on_the_single_runs(runs):
    res = runs.overlapped
    assert res.kge_basins == runs.basins and res.kge.shape == (3, len(runs.basins)) and res.kge.dtype == np.float64
    for k, name in enumerate(res.names):
        q = read_table(os.path.join(runs.single[name], runs.q_file))
        _, ref = skill_np.skill(q, runs.world.area, runs.cells, runs.obs)
        assert np.all((ref >= 0.01) & (ref <= 2.0)), ref
        ed = 1.0 - res.kge[k]
        print(name, 'ED max rel err {:.3e}'.format(float(np.max(np.abs(ed - ref) / ref))))
        assert np.all(np.abs(ed - ref) <= 1e-9 * ref), (name, ed, ref)
    assert not np.array_equal(res.kge[0], res.kge[1]) and not np.array_equal(res.kge[1], res.kge[2])
    lines = open(os.path.join(runs.overlapped_out, 'ensemble', 'member_kge.csv')).read().splitlines()
    assert lines[0] == 'name,' + ','.join(str(b) for b in runs.basins) and len(lines) == 4
    assert [r.split(',')[0] for r in lines[1:]] == res.names
    same_bits(np.array([[float(v) for v in r.split(',')[1:]] for r in lines[1:]]), res.kge, 'member_kge.csv')


def test_member_outputs_0_with_observed_writes_only_the_table(runs):
    from xanthos_amd import run_ensemble
    moved = runs.out + '_serial'
    os.rename(runs.out, moved)
    try:
        res = run_ensemble(runs.ini, members=runs.members, member_outputs=0, observed=runs.obs_rows, obs_unit='km3_per_mth')
        assert sorted(os.listdir(runs.out)) == ['ensemble', 'logfile.log'] and res.member_dirs == [] and res.statistics == {}
        assert os.listdir(os.path.join(runs.out, 'ensemble')) == ['member_kge.csv']
        same_bits(res.kge, runs.overlapped.kge, 'member_outputs = 0')
        assert filecmp.cmp(os.path.join(runs.out, 'ensemble', 'member_kge.csv'),
                           os.path.join(runs.overlapped_out, 'ensemble', 'member_kge.csv'), shallow=False)
    finally:
        shutil.rmtree(runs.out, ignore_errors=True)
        os.rename(moved, runs.out)
