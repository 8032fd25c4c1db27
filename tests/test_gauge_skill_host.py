"""CPU checks of the scoring at stream gauges: the [Evaluate] section and its refusals (each names its key), the loader's
checks, the ensemble plan with gauges, the C-ABI entry in the header, the library and the bindings, and the numpy statement
of the metrics (gauge_skill_np) against a hand-computed case."""
import os
import re
import shutil

import numpy as np
import pytest

import gauge_skill_np
from xanthos_amd import ConfigReader, ValidationException, _hip, ensemble, synth
from xanthos_amd.evaluate import gauge_skill as gskill

NM = 36
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('gskill_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    ini = synth.write_example(root, w, synth.make_forcing(w, NM, seed=50), 1971, 1973, runoff_spinup=25, routing_spinup=6)
    return root, w, ini


def gauge_rows(cells=(5, 17, 17, 60), ids=(11, 12, 13, 14)):
    return np.array([[i, c, 1.0 + k] for k, (i, c) in enumerate(zip(ids, cells))])


def records(ids=(11, 12, 13, 14), nmonths=NM, sentinel=None):
    """Rows [gauge id, 0, 0, value]; gauge 12 has NaN gaps, gauge 13 the sentinel (when given) in every fifth month."""
    rows = []
    for i in ids:
        for m in range(nmonths):
            v = 10.0 + i + 3.0 * np.sin(0.5 * m + i)
            if i == 12 and m % 4 == 0:
                v = np.nan
            if i == 13 and sentinel is not None and m % 5 == 0:
                v = sentinel
            rows.append([i, 0.0, 0.0, v])
    return np.array(rows)


def with_evaluate(ini, tmp_path, gauges=None, obs=None, **kw):
    """A copy of the ini (its input tree stays where it is) with an [Evaluate] section; the two files next to the copy."""
    os.makedirs(str(tmp_path / 'input'), exist_ok=True)
    copy = shutil.copy(ini, str(tmp_path / 'with_evaluate.ini'))
    return synth.enable_evaluate(copy, gauge_rows() if gauges is None else gauges, records() if obs is None else obs, **kw)


def refused(ini, *keys):
    with pytest.raises(ValidationException) as exc:
        c = ConfigReader(ini)
        gskill.load_gauge_set(c)
    msg = str(exc.value)
    assert '[Evaluate]' in msg and all(k in msg for k in keys), msg
    return msg


# ------------------------------------------------------------------ the section
def test_section_is_parsed_and_paths_are_kept_as_written(tree, tmp_path):
    root, w, ini = tree
    assert ConfigReader(ini).evaluate is None
    p = with_evaluate(ini, tmp_path, gauge_missing=-999)
    c = ConfigReader(p)
    assert c.evaluate == {'gauges': str(tmp_path / 'input' / 'eval_gauges.csv'),
                          'gauge_observed': str(tmp_path / 'input' / 'eval_gauge_obs.csv'), 'gauge_missing': -999.0}
    assert c.calibrate == 0 and c.ensemble is None


def test_loader_reads_missing_values_as_nan_and_ignores_weights(tree, tmp_path):
    root, w, ini = tree
    p = with_evaluate(ini, tmp_path, obs=records(sentinel=-999.0), gauge_missing=-999.0)
    gs = gskill.load_gauge_set(ConfigReader(p))
    assert gs.ids.tolist() == [11, 12, 13, 14] and gs.cells.tolist() == [4, 16, 16, 59] and gs.cells.dtype == np.int32
    assert gs.basins.tolist() == [int(w.basin_ids[c]) for c in (4, 16, 16, 59)]
    assert gs.obs.shape == (4, NM) and np.isnan(gs.obs[1, ::4]).all() and np.isnan(gs.obs[2, ::5]).all()
    assert gs.months_used.tolist() == [NM, NM - 9, NM - 8, NM]
    assert not hasattr(gs, 'weights')
    # without the sentinel key the sentinel is a value
    p2 = with_evaluate(ini, tmp_path, obs=records(sentinel=-999.0))
    assert np.isfinite(gskill.load_gauge_set(ConfigReader(p2)).obs[2]).all()
    # the arguments of run_ensemble win over nothing in the ini
    gs3 = gskill.load_gauge_set(ConfigReader(ini), ConfigReader(p).evaluate['gauges'], ConfigReader(p).evaluate['gauge_observed'], -999.0)
    assert np.array_equal(gs3.obs, gs.obs, equal_nan=True)


# ------------------------------------------------------------------ refusals
def test_refuses_a_run_that_does_not_route(tree, tmp_path):
    root, w, ini = tree
    p = with_evaluate(ini, tmp_path)
    text = open(p).read()
    a, b = text.index('[Routing]'), text.index('[Evaluate]')
    open(p, 'w').write(text[:a] + text[b:])
    msg = refused(p, 'routing_module')
    assert 'mrtm' in msg


def test_refuses_half_a_pair_of_keys(tree, tmp_path):
    root, w, ini = tree
    p = with_evaluate(ini, tmp_path)
    text = open(p).read()
    open(p, 'w').write(re.sub(r'\ngauge_observed *=[^\n]*', '', text))
    refused(p, 'gauge_observed')
    open(p, 'w').write(re.sub(r'\ngauges *=[^\n]*', '', text))
    refused(p, 'gauges')
    c = ConfigReader(ini)
    with pytest.raises(ValidationException, match=r'\[Evaluate\] gauge_observed'):
        gskill.load_gauge_set(c, gauges='somewhere.csv')
    with pytest.raises(ValidationException, match=r'\[Evaluate\] gauges'):
        ensemble.validate(c, [('a', {})], gauge_observed='somewhere.csv')


def test_refuses_calibrate_1(tree, tmp_path):
    root, w, ini = tree
    sub = tmp_path / 'cal'
    sub.mkdir()
    obs = np.array([[b, 0.0, 0.0, 1.0 + m] for b in (1, 2) for m in range(NM)])
    cal = synth.write_example(str(sub), w, synth.make_forcing(w, NM, seed=50), 1971, 1973, runoff_spinup=25, routing_spinup=6,
                              obs=obs)
    synth.enable_evaluate(cal, gauge_rows(), records())
    refused(cal, 'Calibrate = 1')


def test_refuses_bad_gauges_and_records(tree, tmp_path):
    root, w, ini = tree
    msg = refused(with_evaluate(ini, tmp_path, gauges=gauge_rows(cells=(5, 17, 17, 61))), 'gauges', 'cell_id 61')
    assert 'gauge 14' in msg
    refused(with_evaluate(ini, tmp_path, gauges=gauge_rows(ids=(11, 12, 12, 14))), 'gauges', 'duplicate gauge id 12')
    one = records()
    one[(one[:, 0] == 11) & (np.arange(len(one)) % NM != 3), 3] = np.nan
    refused(with_evaluate(ini, tmp_path, obs=one), 'gauge_observed', 'gauge 11', '1 finite')
    flat = records()
    flat[flat[:, 0] == 13, 3] = 4.0
    refused(with_evaluate(ini, tmp_path, obs=flat), 'gauge_observed', 'gauge 13', 'zero variance')
    zero = records()
    zero[zero[:, 0] == 14, 3] = np.tile([1.0, -1.0], NM // 2)
    refused(with_evaluate(ini, tmp_path, obs=zero), 'gauge_observed', 'gauge 14', 'zero mean')
    p = with_evaluate(ini, tmp_path)
    os.remove(ConfigReader(p).evaluate['gauge_observed'])
    refused(p, 'gauge_observed', 'does not exist')


# ------------------------------------------------------------------ the ensemble plan
def test_validate_accepts_gauges_alone_and_counts_their_stack(tree, tmp_path):
    root, w, ini = tree
    c = ConfigReader(with_evaluate(ini, tmp_path))
    members = [('a', {}), ('b', {}), ('c', {})]
    with pytest.raises(ValidationException, match='member_outputs'):
        ensemble.validate(ConfigReader(ini), members, member_outputs=0)
    plan = ensemble.validate(c, members, member_outputs=0)                   # gauges alone: the two member tables
    assert plan.gauge_skill.ids.tolist() == [11, 12, 13, 14] and plan.skill is None and plan.statistics_vars == []
    base = ensemble.validate(ConfigReader(ini), members)
    assert base.gauge_skill is None
    ng = 4
    assert plan.bytes_needed == base.bytes_needed + 4 * ng + 8 * ng * (NM + 3 * (NM + 8))
    ensemble.check_fits(plan, plan.bytes_needed)
    with pytest.raises(ValidationException) as exc:
        ensemble.check_fits(plan, plan.bytes_needed - 1)
    assert 'gauges' in str(exc.value) and str(plan.bytes_needed) in str(exc.value)
    ensemble.check_fits(base, 0)                                             # no statistics, no gauges: no stack
    # with statistics the hydrographs' statistics are counted too, and the 64-member limit holds
    stats = ensemble.validate(c, members, statistics=['mean', 'q50'])
    nostat = ensemble.validate(ConfigReader(ini), members, statistics=['mean', 'q50'])
    assert stats.bytes_needed == nostat.bytes_needed + 4 * ng + 8 * ng * (NM + 3 * (NM + 8) + 2 * NM)
    with pytest.raises(ValidationException, match='64'):
        ensemble.validate(c, [('m{}'.format(k), {}) for k in range(65)], statistics=['mean'])
    # the arguments do what the section does
    ev = c.evaluate
    by_args = ensemble.validate(ConfigReader(ini), members, member_outputs=0, gauges=ev['gauges'], gauge_observed=ev['gauge_observed'])
    assert np.array_equal(by_args.gauge_skill.obs, plan.gauge_skill.obs, equal_nan=True)


# ------------------------------------------------------------------ the C-ABI entry
def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'xanthos_hip.h')).read()
    assert re.search(r'\bint xh_gauge_skill\(xh_ctx \*ctx, int64_t ncell, int32_t nmonths, int32_t ngauge,', header)
    assert 'xh_gauge_skill' in _hip.SIGNATURES and len(_hip.SIGNATURES['xh_gauge_skill'][1]) == 9
    assert hasattr(_hip.lib(), 'xh_gauge_skill') and hasattr(_hip.Context, 'gauge_skill')
    assert _hip.lib().xh_abi_version() == _hip.ABI_VERSION


# ------------------------------------------------------------------ the numpy statement, by hand
def test_gauge_skill_np_on_three_months():
    """s = (2, 4, 9), o = (1, 5, NaN-free 6) with a fourth, unobserved month: every column from the definitions."""
    s, o = np.array([2.0, 4.0, 7.0, 9.0]), np.array([1.0, 5.0, np.nan, 6.0])
    row = gauge_skill_np.gauge_row(s, o)
    # V = months 0, 1, 3: s = (2, 4, 9), o = (1, 5, 6); means 5 and 4; population variances 26/3 and 14/3
    r = ((2 - 5) * (1 - 4) + (4 - 5) * (5 - 4) + (9 - 5) * (6 - 4)) / np.sqrt(26.0 * 14.0)
    alpha, beta = np.sqrt(26.0 / 14.0), 5.0 / 4.0
    ed = np.sqrt((r - 1) ** 2 + (alpha - 1) ** 2 + (beta - 1) ** 2)
    sse = 1.0 + 1.0 + 9.0
    ref = np.array([3, ed, r, alpha, beta, 1 - sse / 14.0, 100.0 * 3.0 / 12.0, np.sqrt(sse / 3.0)])
    assert row[0] == 3 and np.allclose(row, ref, rtol=1e-14, atol=0), (row, ref)
    t = gauge_skill_np.table(row)
    assert t['months_used'] == 3 and t['kge'] == 1.0 - row[1] and t['pbias'] == row[6]
    assert list(gskill.COLUMNS) == list(t)
    # one month, or a NaN flow at a scored month: NaN; a NaN flow where nothing was observed: nothing changes
    assert np.isnan(gauge_skill_np.gauge_row(s, np.array([np.nan, 5.0, np.nan, np.nan]))[1:]).all()
    s2 = s.copy()
    s2[2] = np.nan
    assert np.array_equal(gauge_skill_np.gauge_row(s2, o), row)
    s2[0] = np.nan
    assert np.isnan(gauge_skill_np.gauge_row(s2, o)[1:]).all() and gauge_skill_np.gauge_row(s2, o)[0] == 3
    # the product's table of the same columns
    got = gskill.skill_table(row)
    assert all(np.array_equal(got[k], t[k]) for k in t)
