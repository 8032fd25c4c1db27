"""CPU checks of the ensemble run: the [Ensemble] section and every refusal (each names the member and the key), the
resolution of a members-table cell, the numpy restatement of the statistics against numpy itself, the driver's buffer
schedule against a recording stand-in, and that nothing falls back to the host without a device."""
import os
import threading

import numpy as np
import pytest

import ens_np
from xanthos_amd import ConfigReader, ValidationException, _hip, ensemble, synth
from xanthos_amd.components import _FORCING_DATA, _FORCING_SETTINGS
from xanthos_amd.ini_reader import FORCING_SETTINGS, parse_statistic

NM = 36


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('ens_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    forcings = [synth.make_forcing(w, NM, seed=50 + k) for k in range(3)]
    ini, members = synth.write_ensemble_example(root, w, forcings, 1971, 1973, runoff_spinup=25, routing_spinup=6,
                                                statistics=('mean', 'std', 'q10', 'q50'), statistics_vars=('q',))
    return root, w, forcings, ini, members


def plain_ini(ini, tmp_path, extra=''):
    """The tree's ini without its [Ensemble] section (plus ``extra``), as a new file."""
    text = open(ini).read().split('\n[Ensemble]')[0] + extra
    path = str(tmp_path / 'plain.ini')
    with open(path, 'w') as fh:
        fh.write(text)
    return path


def refused(match_member, match_key, config, members, **kw):
    with pytest.raises(ValidationException) as exc:
        ensemble.validate(config, members, **kw)
    msg = str(exc.value)
    assert match_key in msg, msg
    if match_member is not None:
        assert "'{}'".format(match_member) in msg, msg
    return msg


# ------------------------------------------------------------------ the section
def test_section_is_parsed(tree):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    assert c.ensemble == {'members': os.path.join(root, 'input', 'ensemble', 'members.csv'),
                          'statistics': ['mean', 'std', 'q10', 'q50'], 'statistics_vars': ['q'], 'member_outputs': 1}
    assert ConfigReader(ini.replace('.ini', '.ini')).calibrate == 0
    plan = ensemble.validate(c, ensemble.read_members(c, c.ensemble['members']), c.ensemble['statistics'],
                             c.ensemble['statistics_vars'], c.ensemble['member_outputs'])
    assert plan.names == ['m00', 'm01', 'm02'] and plan.statistics_vars == ['q']
    assert plan.statistics == [('mean', None), ('std', None), ('q10', 0.1), ('q50', 0.5)]
    assert plan.ncols == NM and plan.bytes_needed == 8 * 60 * (NM * (3 * 1 + 4) + 2 * NM * (8 + 6))


def test_ini_without_section_has_no_ensemble(tree, tmp_path):
    assert ConfigReader(plain_ini(tree[3], tmp_path)).ensemble is None


def test_statistic_names():
    assert parse_statistic('mean') == ('mean', None) and parse_statistic(' Q07 ') == ('q7', 0.07)
    assert parse_statistic('q100') == ('q100', 1.0) and parse_statistic('q0') == ('q0', 0.0)
    for bad in ('q101', 'median', 'q-1', 'q1.5', 'q', ''):
        with pytest.raises(ValidationException):
            parse_statistic(bad)


def test_bad_section_values(tree, tmp_path):
    for extra, word in (('\n[Ensemble]\nstatistics = mean\n', 'members'),
                        ('\n[Ensemble]\nmembers = m.csv\nstatistics = mean, p50\n', 'p50'),
                        ('\n[Ensemble]\nmembers = m.csv\nmember_outputs = 2\n', 'member_outputs')):
        with pytest.raises(ValidationException, match=word):
            ConfigReader(plain_ini(tree[3], tmp_path, extra))


def test_varying_settings_are_the_forcing_arrays():
    """The settings a member may vary are exactly those behind components._FORCING_DATA, module by module."""
    assert set(FORCING_SETTINGS) == set(_FORCING_DATA) == set(_FORCING_SETTINGS)
    for module, names in _FORCING_DATA.items():
        assert set(names) == set(_FORCING_SETTINGS[module])
        assert {v[0] for v in _FORCING_SETTINGS[module].values()} == set(FORCING_SETTINGS[module])
    assert 'pet_file' not in {k for m in FORCING_SETTINGS.values() for k in m}


def test_csv_cell_resolves_as_the_ini_value(tree):
    """A cell holding the ini's own value gives the ini's own setting, for every forcing setting; an empty cell is left out."""
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    raw = {'pm_tas': 'tas.npy', 'pm_tmin': 'tmin.npy', 'pm_rhs': 'rhs.npy', 'pm_wind': 'wind.npy', 'pm_rsds': 'rsds.npy',
           'pm_rlds': 'rlds.npy', 'PrecipitationFile': os.path.join(root, 'input', 'runoff', 'abcd', 'pr.npy'),
           'TempMinFile': os.path.join(root, 'input', 'runoff', 'abcd', 'tmin.npy')}
    assert set(raw) == set(c.forcing_settings())
    for key, value in raw.items():
        assert c.resolve_forcing_setting(key, value) == getattr(c, key), key
    with pytest.raises(ValidationException, match='StartYear'):
        c.resolve_forcing_setting('StartYear', '1980')
    table = os.path.join(root, 'cells.csv')
    with open(table, 'w') as fh:
        fh.write('name,pm_tas,PrecipitationFile,pm_rhs\nwet,tas.npy,{},\n'.format(raw['PrecipitationFile']))
    assert ensemble.read_members(c, table) == [('wet', {'pm_tas': c.pm_tas, 'PrecipitationFile': c.PrecipitationFile})]
    got = ensemble.read_members(c, c.ensemble['members'])
    assert [(n, {k: os.path.normpath(v) for k, v in o.items()}) for n, o in got] == members


# ------------------------------------------------------------------ refusals
def test_refusals_name_member_and_key(tree, tmp_path):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    good = members[0][1]['PrecipitationFile']
    for key, value in (('StartYear', '1980'), ('ncell', '50'), ('pet_module', 'hs'), ('runoff_spinup', '12'),
                       ('calib_file', good), ('ChStorageFile', good), ('SavFile', good), ('OutputFormat', '4'),
                       ('OutputFolder', 'x'), ('pm_lct', good), ('pet_file', good)):
        refused('b', key, c, [('a', {}), ('b', {key: value})])
    for bad in ('', '  ', 'a/b', '..', '.', 'ensemble', ' pad', os.sep + 'abs'):
        refused(None, 'name', c, [('ok', {}), (bad, {})])
    refused('twin', 'name', c, [('twin', {}), ('twin', {})])
    refused(None, "'name'", c, [{'pm_tas': good}])
    refused(None, 'members', c, [])
    # shapes: an ndarray, and a .npy by its header
    refused('short', 'pm_tas', c, [('short', {'pm_tas': np.zeros((60, NM - 12))})])
    refused('flat', 'PrecipitationFile', c, [('flat', {'PrecipitationFile': np.zeros(60 * NM)})])
    other = str(tmp_path / 'other.npy')
    np.save(other, np.zeros((59, NM)))
    msg = refused('file', 'TempMinFile', c, [('file', {'TempMinFile': other})])
    assert '(59, 36)' in msg and '(60, 36)' in msg
    refused('gone', 'pm_rhs', c, [('gone', {'pm_rhs': str(tmp_path / 'missing.npy')})])
    refused('num', 'pm_rhs', c, [('num', {'pm_rhs': 3.0})])
    # statistics
    refused(None, 'statistics', c, [('a', {})], statistics=['mean', 'q101'])
    refused(None, 'statistics_vars', c, [('a', {})], statistics=['mean'], statistics_vars=['pet'])
    refused(None, 'member_outputs', c, [('a', {})], member_outputs=0)
    refused(None, 'statistics', c, [('m%d' % k, {}) for k in range(65)], statistics=['mean'])
    assert len(ensemble.validate(c, [('m%d' % k, {}) for k in range(65)]).names) == 65      # (no statistics: no limit)
    # several GPUs
    refused(None, 'gpus', c, [('a', {})], gpus=2)


def test_refuses_several_gpus_from_the_environment(tree, monkeypatch):
    c = ConfigReader(tree[3])
    monkeypatch.setenv('XH_GPUS', '2')
    refused(None, 'gpus', c, [('a', {})])
    monkeypatch.delenv('XH_GPUS')
    monkeypatch.setenv('WORLD_SIZE', '2')
    refused(None, 'gpus', c, [('a', {})])
    from xanthos_amd import run_model
    with pytest.raises(ValidationException, match='gpus'):
        run_model(tree[3], gpus=2)


def test_refuses_calibration(tree, tmp_path):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    c.calibrate = 1
    refused(None, 'Calibrate', c, [('a', {})])
    obs = np.stack([np.repeat([1, 2], NM), np.zeros(2 * NM), np.zeros(2 * NM), np.ones(2 * NM)], axis=1)
    cal_ini = synth.write_example(str(tmp_path), w, forcings[0], 1971, 1973, runoff_spinup=25, routing_spinup=6, obs=obs)
    with open(cal_ini, 'a') as fh:
        fh.write('\n[Ensemble]\nmembers = {}\n'.format(os.path.join(root, 'input', 'ensemble', 'members.csv')))
    with pytest.raises(ValidationException, match='Calibrate'):
        ConfigReader(cal_ini)


def test_refuses_stage_by_stage_configurations(tree, tmp_path):
    """What Components.simulation runs on host arrays stage by stage: a PET file (pet_module = none), PM without ABCD."""
    root, w, forcings, ini, members = tree
    text = open(plain_ini(ini, tmp_path)).read()
    head, rest = text.split('[PET]')
    runoff_on = '[Runoff]' + rest.split('[Runoff]')[1]
    pet_file = os.path.join(root, 'input', 'pet', 'penman_monteith', 'tas.npy')
    p1 = str(tmp_path / 'petfile.ini')
    with open(p1, 'w') as fh:
        fh.write(head + '[PET]\npet_module = none\npet_file = {}\n\n'.format(pet_file) + runoff_on)
    msg = refused(None, 'pet_module', ConfigReader(p1), [('a', {})])
    assert 'stage by stage' in msg
    p2 = str(tmp_path / 'pm_only.ini')
    with open(p2, 'w') as fh:
        fh.write(text.split('[Runoff]')[0] + '[Routing]' + text.split('[Routing]')[1])
    refused(None, 'runoff_module', ConfigReader(p2), [('a', {})])


def test_refuses_a_stack_beyond_the_free_memory(tree):
    c = ConfigReader(tree[3])
    plan = ensemble.validate(c, [('a', {}), ('b', {})], statistics=['mean'])
    ensemble.check_fits(plan, plan.bytes_needed)
    with pytest.raises(ValidationException) as exc:
        ensemble.check_fits(plan, plan.bytes_needed - 1)
    assert 'statistics' in str(exc.value) and str(plan.bytes_needed) in str(exc.value) and str(plan.bytes_needed - 1) in str(exc.value)
    ensemble.check_fits(ensemble.validate(c, [('a', {})]), 0)          # no statistics: no stack


# ------------------------------------------------------------------ the statistics, restated, against numpy
@pytest.mark.parametrize('S', [1, 2, 3, 17, 64])
def test_ens_np_equals_numpy(S):
    x = ens_np.stack(7 * S, S, 3001, nan_share=0.02)
    assert np.isnan(x).any() and not np.isnan(x).all(axis=0).all()
    for name in ('mean', 'std', 'min', 'max', 'q0', 'q10', 'q50', 'q90', 'q100', 'q37'):
        got, ref = ens_np.stat(x, name), ens_np.numpy_stat(x, name)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (S, name)
        m = ~np.isnan(ref)
        assert np.array_equal(got[m], ref[m]), (S, name, int((got[m] != ref[m]).sum()))
        assert S == 1 and name == 'std' or m.any()


# ------------------------------------------------------------------ the buffer schedule
class Recorder:
    """Stand-in for the pipeline's three stages: records begin / end of each with a global clock."""

    def __init__(self, fail_at=None):
        self.lock, self.events, self.fail_at = threading.Lock(), [], fail_at

    def stage(self, kind):
        def call(k, i):
            with self.lock:
                self.events.append((kind, 'begin', k, i, threading.current_thread().name))
            if self.fail_at == (kind, k):
                raise RuntimeError('stage {} of member {} failed'.format(kind, k))
            with self.lock:
                self.events.append((kind, 'end', k, i, threading.current_thread().name))
        return call

    def at(self, kind, edge, k):
        return next(n for n, e in enumerate(self.events) if e[:3] == (kind, edge, k))


@pytest.mark.parametrize('n', [1, 2, 3, 7])
def test_overlapped_schedule_orders_buffer_sets(n):
    for _ in range(20):                                   # (the interleaving varies from run to run)
        r = Recorder()
        ensemble.run_schedule(n, r.stage('upload'), r.stage('compute'), r.stage('write'), overlap=True)
        assert len(r.events) == 6 * n
        for kind in ('upload', 'compute', 'write'):
            assert [e[2] for e in r.events if e[0] == kind and e[1] == 'begin'] == list(range(n))      # member order
            assert all(e[3] == e[2] % 2 for e in r.events if e[0] == kind)                              # two sets, alternating
            assert len({e[4] for e in r.events if e[0] == kind}) == 1                                   # one host thread per stage
        assert len({e[4] for e in r.events}) == 3
        for k in range(n):
            assert r.at('upload', 'end', k) < r.at('compute', 'begin', k)       # never computed before its upload completed
            assert r.at('compute', 'end', k) < r.at('write', 'begin', k)
            if k >= 2:
                assert r.at('compute', 'end', k - 2) < r.at('upload', 'begin', k)      # the forcing of the set was read
                assert r.at('write', 'end', k - 2) < r.at('compute', 'begin', k)       # the outputs of the set were written


def test_serial_schedule_is_one_after_the_other():
    r = Recorder()
    ensemble.run_schedule(3, r.stage('upload'), r.stage('compute'), r.stage('write'), overlap=False)
    assert [(e[0], e[2], e[3]) for e in r.events if e[1] == 'begin'] == \
        [(kind, k, 0) for k in range(3) for kind in ('upload', 'compute', 'write')]
    assert len({e[4] for e in r.events}) == 1


@pytest.mark.parametrize('where', [('upload', 1), ('compute', 0), ('write', 2)])
def test_schedule_raises_the_first_failure_and_ends(where):
    r = Recorder(fail_at=where)
    with pytest.raises(RuntimeError, match='stage {} of member {}'.format(*where)):
        ensemble.run_schedule(5, r.stage('upload'), r.stage('compute'), r.stage('write'), overlap=True)
    assert not [t for t in threading.enumerate() if t.name.startswith('xh-ens-')]
    assert not [e for e in r.events if e[0] == 'write' and e[2] > where[1] + 2]


# ------------------------------------------------------------------ no host fallback
def test_run_ensemble_needs_a_device(tree):
    if _hip.device_count() > 0:
        pytest.skip('a GPU is present')
    from xanthos_amd import Xanthos, run_ensemble, run_model
    with pytest.raises(_hip.HipUnavailable):
        run_ensemble(tree[3])
    with pytest.raises(_hip.HipUnavailable):
        run_model(tree[3])
    with pytest.raises(_hip.HipUnavailable):
        Xanthos(tree[3]).execute_ensemble([('a', {'PrecipitationFile': tree[2][1]['precip']})], statistics=['mean'])
    out = os.path.join(tree[0], 'output', 'pm_abcd_mrtm_synth')
    assert sorted(os.listdir(out)) == ['logfile.log']                  # nothing was computed or written on the host
