"""GPU tests (-m gpu) of the ensemble run: xh_ens_stats through the C-ABI against numpy, bit for bit, and
run_ensemble() on small synthetic worlds -- members byte-identical to single runs, the overlapped schedule equal to the
serial one, the statistics equal to numpy over the stacked member outputs, member_outputs = 0, and the resident state
(one routing plan for all members; a plain run afterwards unchanged)."""
import filecmp
import os

import numpy as np
import pytest

import ens_np

pytestmark = pytest.mark.gpu

QS = (0.0, 0.1, 0.5, 0.9, 1.0)
NAMES = ('mean', 'std', 'min', 'max')


def same_bits(x, ref, tag=''):
    x, ref = np.asarray(x), np.asarray(ref)
    assert x.shape == ref.shape, tag
    assert np.array_equal(np.isnan(x), np.isnan(ref)), 'NaN masks differ ' + str(tag)
    m = ~np.isnan(ref)
    assert np.array_equal(x[m], ref[m]), '{}: {} of {} values differ'.format(tag, int((x[m] != ref[m]).sum()), int(m.sum()))


# ------------------------------------------------------------------ 4. the kernel through the C-ABI
# every S of the issue at every n (one lane, a wave less one, a wave, a wave and one, several workgroups, an odd size of many
# workgroups), and at one n the member counts at which the library changes kernel: 2 | 3-4 | 5-8 | 9-16 in registers, 17+ in LDS
CASES = [(S, n) for S in (1, 2, 3, 17, 64) for n in (1, 63, 64, 65, 257, 100003)] + [(S, 257) for S in (4, 5, 8, 9, 16, 33)]


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


@pytest.mark.parametrize('S,n', CASES)
def test_ens_stats_equals_numpy(ctx, S, n):
    x = ens_np.stack(1000 * S + n, S, n)
    members = [ctx.upload(x[j]) for j in range(S)]
    outs = [ctx.empty((n,)) for _ in range(len(NAMES) + len(QS))]
    ctx.ens_stats(n, members, NAMES, QS, outs)                      # all statistics in one call
    got = [o.download() for o in outs]
    # numpy adds the rows of a [S, n] stack in member order -- except for n = 1, where the reduction runs along contiguous
    # memory and np.add.reduce switches to its pairwise order (8 accumulators) from S = 8 on.  The definition is the member
    # order, so numpy is shown the single element twice (a [S, 2] stack) and its first column is taken.
    xn = x if n > 1 else np.repeat(x, 2, axis=1)
    ref = [ens_np.numpy_stat(xn, k)[:n] for k in NAMES] + [np.quantile(xn, q, axis=0, method='linear')[:n] for q in QS]
    own = [ens_np.stat(x, k) for k in NAMES] + [ens_np.quantile(x, q) for q in QS]
    for tag, g, r, o in zip(NAMES + tuple('q%g' % q for q in QS), got, ref, own):
        same_bits(g, r, (S, n, tag, 'numpy'))
        same_bits(g, o, (S, n, tag, 'ens_np'))
    if n >= 4:
        assert np.isnan(got[0][n - 1]) and np.isnan(got[-1][n // 4])      # all members NaN / the first member NaN
    one = ctx.empty((n,))
    for k, name in enumerate(NAMES):                                # one statistic per call: the same bits
        ctx.ens_stats(n, members, (name,), (), [one])
        same_bits(one.download(), got[k], (S, n, name, 'alone'))
    for k, q in enumerate(QS):
        ctx.ens_stats(n, members, (), (q,), [one])
        same_bits(one.download(), got[len(NAMES) + k], (S, n, q, 'alone'))
    for a in members + outs + [one]:
        a.free()


def test_ens_stats_limits_and_arguments(ctx):
    from xanthos_amd import _hip
    a, out = ctx.upload(np.arange(8.0)), ctx.empty((8,))
    with pytest.raises(_hip.HipError, match='error {}'.format(_hip.XH_ERR_LIMIT)):
        ctx.ens_stats(8, [a] * 65, ('mean',), (), [out])
    with pytest.raises(_hip.HipError, match='error {}'.format(_hip.XH_ERR_LIMIT)):
        ctx.ens_stats(8, [a] * 3, (), [0.5] * 17, [out] * 17)
    for members, outs in (([a, None], [out]), ([a, a], [None])):
        with pytest.raises(_hip.HipError, match='error {}'.format(_hip.XH_ERR_ARG)):
            ctx.ens_stats(8, members, ('mean',), (), outs)
    with pytest.raises(_hip.HipError, match='error {}'.format(_hip.XH_ERR_ARG)):
        ctx.ens_stats(8, [a, a], (), (1.5,), [out])
    with pytest.raises(_hip.HipError, match='error {}'.format(_hip.XH_ERR_ARG)):
        ctx._check(_hip.lib().xh_ens_stats(ctx.handle, 8, 2, None, 1, 0, None, None))
    ctx.ens_stats(8, [a] * 64, ('max',), (), [out])                 # the limit itself is served
    assert np.array_equal(out.download(), np.arange(8.0))
    a.free()
    out.free()


# ------------------------------------------------------------------ the driver on small synthetic worlds
S = 5
STATS = ('mean', 'std', 'min', 'max', 'q10', 'q50', 'q90')
PROJECT = 'pm_abcd_mrtm_synth'


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


def make_tree(root, years=3, seed=33, **kw):
    from xanthos_amd import synth
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=seed)
    forcings = [synth.make_forcing(w, 12 * years, seed=100 + 7 * k) for k in range(S)]      # (0.1 % of the cells without precipitation)
    ini, members = synth.write_ensemble_example(root, w, forcings, 1971, 1970 + years, runoff_spinup=25, routing_spinup=6,
                                                statistics=STATS, **kw)
    return SimpleTree(root=root, world=w, forcings=forcings, ini=ini, members=members,
                      out=os.path.join(root, 'output', PROJECT))


class SimpleTree:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def check_statistics(tree, result, ext, unit, nvars=('q', 'avgchflow')):
    """Every written var x stat file equals numpy over the stacked member files, bit for bit; so does the result object."""
    for var in nvars:
        u = 'm3persec' if var == 'avgchflow' else unit
        stack = np.stack([read_table(os.path.join(tree.out, name, '{}_{}_{}.{}'.format(var, u, PROJECT, ext)))
                          for name, _ in tree.members])
        for stat in STATS:
            got = read_table(os.path.join(tree.out, 'ensemble', '{}_{}_{}_{}.{}'.format(var, u, PROJECT, stat, ext)))
            ref = ens_np.numpy_stat(stack, stat)
            for a in (got, ref):
                assert np.isnan(a).mean() < 0.05, (var, stat, float(np.isnan(a).mean()))
            same_bits(got, ref, (var, stat, 'file'))
            same_bits(result.statistics[var][stat], ref, (var, stat, 'result'))


CONFIGS = {'csv_month_mm': dict(output_format=1, output_in_year=0, output_unit=0),
           'npy_year_km3': dict(output_format=4, output_in_year=1, output_unit=1),
           'npy_month_km3': dict(output_format=4, output_in_year=0, output_unit=1),
           'csv_year_mm': dict(output_format=1, output_in_year=1, output_unit=0),
           'npy_month_mm': dict(output_format=4, output_in_year=0, output_unit=0)}


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_members_equal_single_runs_and_statistics_equal_numpy(tmp_path, name):
    """1 + 3: run_model on an ini with [Ensemble]; every member's folder against a single run with the same overrides."""
    from xanthos_amd import Xanthos, run_model
    tree = make_tree(str(tmp_path), **CONFIGS[name])
    res = run_model(tree.ini)
    assert res.names == [n for n, _ in tree.members] and res.member_dirs == [os.path.join(tree.out, n) for n in res.names]
    assert all(len(res.timings[k]) == S for k in ('upload', 'kernels', 'post', 'write')) and res.timings['statistics'] > 0
    for member, overrides in tree.members:
        ref = os.path.join(str(tmp_path), 'single', member)
        Xanthos(tree.ini).execute(dict(overrides, OutputFolder=ref))
        same_files(os.path.join(tree.out, member), ref, member)
    assert sorted(os.listdir(tree.out)) == sorted(['ensemble', 'logfile.log'] + res.names)
    cfg = CONFIGS[name]
    check_statistics(tree, res, 'npy' if cfg['output_format'] == 4 else 'csv',
                     '{}per{}'.format(('mm', 'km3')[cfg['output_unit']], ('month', 'year')[cfg['output_in_year']]))


def test_post_processors_aggregates_and_in_memory_member(tmp_path):
    """1: drought, accessible water and the three spatial aggregates per member; one member given as ndarrays."""
    from xanthos_amd import Xanthos, run_ensemble
    tree = make_tree(str(tmp_path), years=6, seed=34, post=True, aggregates=True, output_format=4, section=False)
    members = list(tree.members)
    keys = {'pm_tas': 'tas', 'pm_tmin': 'tmin', 'pm_rhs': 'rhs', 'pm_wind': 'wind', 'pm_rsds': 'rsds', 'pm_rlds': 'rlds',
            'PrecipitationFile': 'precip', 'TempMinFile': 'abcd_tmin'}
    members[2] = {'name': members[2][0], **{k: tree.forcings[2][v] for k, v in keys.items()}}       # in memory, as a dict
    members[4] = (members[4][0], {'PrecipitationFile': members[4][1]['PrecipitationFile']})          # the rest: the ini's
    res = run_ensemble(tree.ini, members=members, statistics=['mean', 'q50'], statistics_vars=['q'])
    for member, overrides in (tree.members[0], tree.members[2], members[4]):
        ref = os.path.join(str(tmp_path), 'single', member)
        Xanthos(tree.ini).execute(dict(overrides, OutputFolder=ref))
        same_files(os.path.join(tree.out, member), ref, member)
        names = sorted(files_of(ref))
        assert any(n.startswith('drought_thresholds') for n in names) and any(n.startswith('accessible_water') for n in names)
        assert sum(n.split('_')[0] in ('Basin', 'Country', 'GCAMRegion') for n in names) == 3
    assert sorted(res.statistics) == ['q'] and sorted(res.statistics['q']) == ['mean', 'q50']
    assert sorted(os.listdir(os.path.join(tree.out, 'ensemble'))) == sorted(
        'q_mmpermonth_{}_{}.npy'.format(PROJECT, s) for s in ('mean', 'q50'))


def test_overlap_changes_no_bit_and_member_outputs_0(tmp_path):
    """2 + 5: the overlapped and the serial schedule give identical files and statistics; member_outputs = 0 writes only
    ensemble/, with the same statistics."""
    from xanthos_amd import run_ensemble
    tree = make_tree(str(tmp_path), output_format=4, output_in_year=1)
    a = run_ensemble(tree.ini, overlap=True)
    stats_a = {v: {s: a.statistics[v][s] for s in STATS} for v in ('q', 'avgchflow')}
    kept = tree.out + '_overlapped'
    os.rename(tree.out, kept)
    b = run_ensemble(tree.ini, overlap=False)
    same_files(kept, tree.out, 'overlap')
    for v in stats_a:
        for s in STATS:
            same_bits(b.statistics[v][s], stats_a[v][s], (v, s))
    os.rename(tree.out, tree.out + '_serial')
    c = run_ensemble(tree.ini, member_outputs=0)
    assert sorted(os.listdir(tree.out)) == ['ensemble', 'logfile.log'] and c.member_dirs == []
    same_files(os.path.join(tree.out, 'ensemble'), os.path.join(kept, 'ensemble'), 'member_outputs = 0')
    for v in stats_a:
        for s in STATS:
            same_bits(c.statistics[v][s], stats_a[v][s], (v, s, 'member_outputs = 0'))


def test_resident_state(tmp_path, monkeypatch):
    """6: one routing plan for all members, and a plain run afterwards writes what it wrote before."""
    from xanthos_amd import _hip, components, run_ensemble, run_model
    tree = make_tree(str(tmp_path), seed=36, output_format=4, section=False)
    before = os.path.join(str(tmp_path), 'before')
    run_model(tree.ini)
    os.rename(tree.out, before)
    components._TOPOLOGIES.clear()                         # (the plain run's plan: the ensemble has to make its own)
    made = []
    create = _hip.Context.route_plan
    monkeypatch.setattr(_hip.Context, 'route_plan', lambda self, *a: made.append(1) or create(self, *a))
    res = run_ensemble(tree.ini, members=tree.members, statistics=['mean'])
    assert len(res.names) == S and len(made) == 1, made    # xh_route_plan_create (the partition) ran once for S members
    (dsid, upid, um), = components._TOPOLOGIES.values()
    assert len(um._plans) == 1
    for name in res.names:
        os.rename(os.path.join(tree.out, name), os.path.join(str(tmp_path), 'member_' + name))
    os.rename(os.path.join(tree.out, 'ensemble'), os.path.join(str(tmp_path), 'stats'))
    run_model(tree.ini)
    assert len(made) == 1                                  # ... and the plain run found it
    same_files(tree.out, before, 'plain run after the ensemble')
