"""CPU checks of the parameter ensemble: the member key abcd_pars and its refusals (each names the member and the key), the
resident plan, the members table's abcd_pars column, the [Ensemble] observed / obs_unit keys and their refusals, and the
numpy restatement of the member skill against a hand-written distance."""
import os

import numpy as np
import pytest

import skill_np
from xanthos_amd import ConfigReader, ValidationException, ensemble, synth

NM = 36


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('pens_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    forcings = [synth.make_forcing(w, NM, seed=50 + k) for k in range(2)]
    ini, members = synth.write_ensemble_example(root, w, forcings, 1971, 1973, runoff_spinup=25, routing_spinup=6, section=False)
    return root, w, forcings, ini, members


def refused(match_member, match_key, config, members, **kw):
    with pytest.raises(ValidationException) as exc:
        ensemble.validate(config, members, **kw)
    msg = str(exc.value)
    assert match_key in msg, msg
    if match_member is not None:
        assert "'{}'".format(match_member) in msg, msg
    return msg


def observations(w, nmonths=NM, basins=None):
    """Rows [basin id, 0, 0, value], months in order, basin after basin."""
    basins = sorted(set(int(b) for b in w.basin_ids)) if basins is None else basins
    return np.array([[b, 0.0, 0.0, 1.0 + 0.1 * b + 0.01 * m] for b in basins for m in range(nmonths)])


# ------------------------------------------------------------------ accepted input, and the plan
def test_abcd_pars_is_accepted_and_the_plan_is_resident(tree, tmp_path):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    table = np.load(c.calib_file)
    path = str(tmp_path / 'other_pars.npy')
    np.save(path, table * 0.99)
    plan = ensemble.validate(c, [('own', {}), ('array', {'abcd_pars': table * 1.01}), ('file', {'abcd_pars': path}),
                                 ('ints', {'abcd_pars': np.ones(table.shape, dtype=np.int64)})], statistics=['mean'])
    assert plan.resident and plan.names == ['own', 'array', 'file', 'ints']
    assert plan.overrides[0] == {} and plan.overrides[2] == {'abcd_pars': path}
    # one forcing set (8 arrays), two output sets that share the one PET (11), the stack of 4 members x 2 variables, 1 statistic
    assert plan.bytes_needed == 8 * 60 * (NM * (4 * 2 + 1) + NM * (8 + 2 * 6 - 1))
    mixed = ensemble.validate(c, [('own', {}), ('wet', {'abcd_pars': table, 'PrecipitationFile': members[1][1]['PrecipitationFile']})],
                              statistics=['mean'])
    assert not mixed.resident
    assert mixed.bytes_needed == 8 * 60 * (NM * (2 * 2 + 1) + 2 * NM * (8 + 6))
    assert not ensemble.validate(c, members).resident
    assert ensemble.validate(c, [('a', {}), ('b', {})]).resident          # (nothing varies: still one upload)


def test_abcd_pars_refusals_name_member_and_key(tree, tmp_path):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    table = np.load(c.calib_file)
    msg = refused('short', 'abcd_pars', c, [('ok', {}), ('short', {'abcd_pars': table[:-1]})])
    assert str(table[:-1].shape) in msg and str(table.shape) in msg
    refused('flat', 'abcd_pars', c, [('flat', {'abcd_pars': table.reshape(-1)})])
    other = str(tmp_path / 'four.npy')
    np.save(other, table[:, :4])
    msg = refused('file', 'abcd_pars', c, [('file', {'abcd_pars': other})])
    assert str(table[:, :4].shape) in msg and str(table.shape) in msg
    refused('gone', 'abcd_pars', c, [('gone', {'abcd_pars': str(tmp_path / 'missing.npy')})])
    refused('num', 'abcd_pars', c, [('num', {'abcd_pars': 3.0})])
    refused('text', 'abcd_pars', c, [('text', {'abcd_pars': np.full(table.shape, 'a')})])
    refused('cplx', 'abcd_pars', c, [('cplx', {'abcd_pars': table.astype(complex)})])


def test_abcd_pars_needs_abcd(tmp_path):
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = synth.hgm_forcing(w, synth.make_forcing(w, NM, seed=50))
    ini = synth.write_hgm_example(str(tmp_path), w, f, 1971, 1973)
    c = ConfigReader(ini)
    assert (c.pet_module, c.runoff_module) == ('hargreaves', 'gwam')
    refused('p', 'abcd_pars', c, [('own', {}), ('p', {'abcd_pars': w.abcd_pars})])


def test_calib_file_is_still_refused_and_points_to_abcd_pars(tree):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    msg = refused('b', 'calib_file', c, [('a', {}), ('b', {'calib_file': c.calib_file})])
    assert 'abcd_pars' in msg
    assert 'abcd_pars' not in refused('b', 'StartYear', c, [('a', {}), ('b', {'StartYear': '1980'})])


# ------------------------------------------------------------------ the members table
def test_members_csv_resolves_abcd_pars_against_the_runoff_directory(tree, tmp_path):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    np.save(os.path.join(c.ro_model_dir, 'set_b.npy'), np.load(c.calib_file) * 1.02)
    absolute = str(tmp_path / 'set_c.npy')
    np.save(absolute, np.load(c.calib_file) * 0.98)
    table = str(tmp_path / 'members.csv')
    with open(table, 'w') as fh:
        fh.write('name,abcd_pars,PrecipitationFile\nown,,\nb,set_b.npy,\nc,{},{}\n'.format(
            absolute, members[1][1]['PrecipitationFile']))
    got = ensemble.read_members(c, table)
    assert got == [('own', {}), ('b', {'abcd_pars': os.path.join(c.ro_model_dir, 'set_b.npy')}),
                   ('c', {'abcd_pars': absolute, 'PrecipitationFile': members[1][1]['PrecipitationFile']})]
    assert os.path.dirname(got[1][1]['abcd_pars']) == os.path.dirname(c.calib_file)       # as calib_file resolves
    assert not ensemble.validate(c, got).resident
    assert ensemble.validate(c, got[:2]).resident


# ------------------------------------------------------------------ observed / obs_unit
def test_section_keys_observed_and_obs_unit(tree, tmp_path):
    root, w, forcings, ini, members = tree
    obs_file = os.path.join(root, 'input', 'obs_runoff.csv')
    np.savetxt(obs_file, observations(w), delimiter=',', fmt='%.17g')
    table = os.path.join(root, 'input', 'ensemble', 'members.csv')
    path = str(tmp_path / 'with_obs.ini')
    with open(path, 'w') as fh:
        fh.write(open(ini).read() + '\n[Ensemble]\nmembers = {}\nobserved = input/obs_runoff.csv\nobs_unit = mm_per_mth\n'.format(table))
    c = ConfigReader(path)
    assert c.ensemble['observed'] == obs_file and c.ensemble['obs_unit'] == 'mm_per_mth'
    plan = ensemble.validate(c, members, observed=c.ensemble['observed'], obs_unit=c.ensemble['obs_unit'])
    basins = sorted(set(int(b) for b in w.basin_ids))
    assert plan.skill.basins == basins and plan.skill.unit == 'mm_per_mth' and plan.skill.obs.shape == (len(basins), NM)
    for j, b in enumerate(basins):
        lo, hi = plan.skill.start[j], plan.skill.start[j + 1]
        assert np.array_equal(plan.skill.cells[lo:hi], np.flatnonzero(w.basin_ids == b))
        assert np.array_equal(plan.skill.obs[j], 1.0 + 0.1 * b + 0.01 * np.arange(NM))
    assert plan.skill.start.dtype == np.int64 and plan.skill.cells.dtype == np.int32
    with open(path, 'w') as fh:
        fh.write(open(ini).read() + '\n[Ensemble]\nmembers = {}\nobs_unit = mm_per_mth\n'.format(table))
    with pytest.raises(ValidationException, match='observed'):
        ConfigReader(path)


def test_observed_refusals(tree):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    obs = observations(w)
    refused(None, 'obs_unit', c, [('a', {})], observed=obs)
    refused(None, 'obs_unit', c, [('a', {})], observed=obs, obs_unit='m3_per_sec')
    absent = max(int(b) for b in w.basin_ids) + 1
    msg = refused(None, 'observed', c, [('a', {})], observed=np.concatenate([obs, observations(w, basins=[absent])]),
                  obs_unit='km3_per_mth')
    assert 'basin {}'.format(absent) in msg
    first = int(obs[0, 0])
    msg = refused(None, 'observed', c, [('a', {})], observed=obs[1:], obs_unit='km3_per_mth')      # one month short
    assert 'basin {}'.format(first) in msg and str(NM - 1) in msg
    refused(None, 'observed', c, [('a', {})], observed=obs[:, :3], obs_unit='km3_per_mth')
    # a longer record is allowed: its first nmonths are used
    longer = observations(w, nmonths=NM + 5)
    plan = ensemble.validate(c, [('a', {})], observed=longer, obs_unit='km3_per_mth')
    assert np.array_equal(plan.skill.obs, ensemble.validate(c, [('a', {})], observed=obs, obs_unit='km3_per_mth').skill.obs)


def test_observed_needs_a_runoff_module(tmp_path):
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = synth.hgm_forcing(w, synth.make_forcing(w, NM, seed=50))
    ini = synth.write_hgm_example(str(tmp_path), w, f, 1971, 1973)
    text = open(ini).read()
    with open(ini, 'w') as fh:                            # Hargreaves PET and routing, no [Runoff]
        fh.write(text.split('[Runoff]')[0] + '[Routing]' + text.split('[Routing]')[1])
    c = ConfigReader(ini)
    assert c.runoff_module == 'none'
    refused(None, 'observed', c, [('a', {})], observed=observations(w), obs_unit='km3_per_mth')


def test_member_outputs_0_with_observed_alone(tree):
    root, w, forcings, ini, members = tree
    c = ConfigReader(ini)
    refused(None, 'member_outputs', c, [('a', {})], member_outputs=0)
    plan = ensemble.validate(c, [('a', {})], member_outputs=0, observed=observations(w), obs_unit='km3_per_mth')
    assert plan.member_outputs == 0 and plan.statistics_vars == [] and plan.skill is not None


# ------------------------------------------------------------------ the helper, by hand
def test_skill_np_against_a_hand_written_distance():
    q = np.array([[1.0, 2.0, 6.0], [3.0, np.nan, 2.0], [100.0, 100.0, 100.0], [np.nan, np.nan, np.nan]])
    area = np.array([2.0e6, 1.0e6, 5.0, 7.0])
    obs = np.array([[4.0, 5.0, 12.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])
    series, ed = skill_np.skill(q, area, [np.array([0, 1]), np.array([2]), np.array([3])], obs, 'km3_per_mth')
    s = np.array([1.0 * 2.0 + 3.0 * 1.0, 2.0 * 2.0, 6.0 * 2.0 + 2.0 * 1.0])       # the NaN term adds nothing
    assert np.allclose(series[0], s, rtol=1e-15, atol=0) and np.array_equal(series[2], np.zeros(3))
    o = obs[0]
    ms, mo = s.sum() / 3, o.sum() / 3
    ss, so = (((s - ms) ** 2).sum() / 3) ** 0.5, (((o - mo) ** 2).sum() / 3) ** 0.5
    r = ((s - ms) * (o - mo)).sum() / 3 / (ss * so)
    hand = ((r - 1) ** 2 + (ss / so - 1) ** 2 + (ms / mo - 1) ** 2) ** 0.5
    assert abs(ed[0] - hand) <= 1e-14 * hand and 0.01 < hand < 2
    assert np.isnan(ed[1]) and np.isnan(ed[2])            # a constant series; a basin whose Q is NaN everywhere
    plain, _ = skill_np.skill(q, None, [np.array([0, 1])], obs[:1], 'mm_per_mth')
    assert np.array_equal(plain[0], [4.0, 2.0, 8.0])
    assert [list(c) for c in skill_np.cells_of([2, 1, 2, 3], [1, 2])] == [[1], [0, 2]]
