"""CPU checks of the streamflow calibration objective (set_calibrate = 1): the numpy restatement against the golden made
with the reference's own parts, the host tables (outlets, closures, local CSR) on hand-built graphs and on the golden
world, and the refusals (no MRTM, NaN forcing, a closure too large)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import scipy.sparse as sparse

import flowcal_np
from xanthos_amd.calibrate import flow_tables as ft
from xanthos_amd.calibrate.calibrate_abcd import Calibrate, calibrate_all
from xanthos_amd.ini_reader import ValidationException, check_modules


def _um(g):
    return sparse.csr_matrix((g['data'].astype(int), g['indices'], g['indptr']), shape=(g['indptr'].size - 1,) * 2)


def _graph(n, edges):
    """UM = UP - I of a network given as (from, to) edges: row `to` holds +1 at column `from`."""
    r = [t for f, t in edges] + list(range(n))
    c = [f for f, t in edges] + list(range(n))
    v = [1] * len(edges) + [-1] * n
    m = sparse.csr_matrix((v, (r, c)), shape=(n, n))
    m.sort_indices()
    return m


@pytest.mark.parametrize('tag', ['snow', 'nosnow'])
def test_numpy_restatement_matches_reference_golden(golden, tag):
    g = golden('flowcal')
    um = _um(g)
    nm, spin, rspin = int(g['nmonths']), int(g['runoff_spinup']), int(g['routing_spinup'])
    tmin = g['tmin'] if tag == 'snow' else None
    npar = 5 if tmin is not None else 4
    for i, b in enumerate(g['basins']):
        cells = np.nonzero(g['basin_ids'] == b)[0]
        for j, p in enumerate(g['pars']):
            ed, s = flowcal_np.objective(p[:npar], g[tag + '_obs'][i], cells, um, g['pet'], g['precip'], tmin,
                                         g['flow_dist'], g['velocity'], g['area'], g['chs_prev'], g['ndays'], nm, spin,
                                         rspin, dt=float(g['dt']))
            ref = g[tag + '_series'][i, j]
            assert np.all(np.abs(s - ref) <= 1e-12 * np.abs(ref)), (b, j, np.max(np.abs(s - ref) / np.abs(ref)))
            assert abs(ed - g[tag + '_ed'][i, j]) <= 1e-12 * max(1.0, abs(ed)), (b, j)


def test_golden_world_covers_the_corners(golden):
    """The golden holds a 1-cell basin, a basin with several outlets, a closure with foreign cells, and firing cells."""
    g = golden('flowcal')
    um = _um(g)
    t = ft.FlowTables(um, g['basin_ids'], list(g['basins']), g['flow_dist'], g['velocity'], g['area'], g['chs_prev'],
                      g['ndays'], int(g['nmonths']), int(g['routing_spinup']))
    sizes = {b: (g['basin_ids'] == b).sum() for b in g['basins']}
    assert sizes[9] == 1
    assert max(len(o) for o in t.outlets) > 1
    assert any(c.size > (g['basin_ids'] == b).sum() for b, c in zip(t.basins, t.closures))
    assert (g['velocity'] * float(g['dt']) > g['flow_dist']).sum() > 10


def test_outlets_and_closures_on_hand_built_graphs():
    # 0 -> 1 -> 2 -> (ocean);  3 -> 2;  4 -> (ocean);  5 -> 3 (a foreign tributary);  6, 7 unconnected
    edges = [(0, 1), (1, 2), (3, 2), (5, 3)]
    um = _graph(8, edges)
    ip, ix, sg = ft.um_arrays(um)
    out, clo = ft.outlets_and_closure(ip, ix, sg, np.array([0, 1, 2, 3, 4]))
    assert out.tolist() == [2, 4]                          # two outlets: the river mouth and a coastal cell
    assert clo.tolist() == [0, 1, 2, 3, 4, 5]              # the foreign tributary 5 is in the closure
    out, clo = ft.outlets_and_closure(ip, ix, sg, np.array([5]))
    assert out.tolist() == [5] and clo.tolist() == [5]     # drains into another basin: an outlet of its own basin
    out, clo = ft.outlets_and_closure(ip, ix, sg, np.array([4]))
    assert out.tolist() == [4] and clo.tolist() == [4]     # a 1-cell basin
    # 6 and 7 share no edge of UM: two outlets, two closures of their own
    out, clo = ft.outlets_and_closure(ip, ix, sg, np.array([6, 7]))
    assert out.tolist() == [6, 7] and clo.tolist() == [6, 7]


def test_tables_follow_um_not_dsid_across_the_date_line():
    """A cell in the last column that flows east: downstream() wraps it to a cell of the same row (mrtm.py:100-102),
    upstream() scans neighbours without wrapping (:150), so UM drops that edge.  The outlets and the closure follow UM."""
    from xanthos_amd.routing import mrtm
    st = NS(ngridrow=3, ngridcol=4)
    # id, lon, lat, column (1-based), row (1-based): A at the east edge, B two columns further on across the line
    coords = np.array([[1, 0, 0, 4, 2], [2, 0, 0, 2, 2], [3, 0, 0, 1, 2]], dtype=float)
    flow_dir = np.array([1.0, 16.0, 0.0])                  # A east (wraps), B west into C, C no direction
    dsid = mrtm.downstream(coords, flow_dir, st)
    assert dsid.tolist() == [2, 3, -1]                      # dsid: A -> B -> C
    um = mrtm.upstream_genmatrix(mrtm.upstream(coords, dsid, st))
    ip, ix, sg = ft.um_arrays(um)
    assert um.tocsr()[1, 0] == 0 and um.tocsr()[2, 1] == 1  # UM: B -> C kept, A -> B dropped
    out, clo = ft.outlets_and_closure(ip, ix, sg, np.array([0, 1]))
    assert out.tolist() == [0, 1] and clo.tolist() == [0, 1]    # by dsid A would drain into B and not be an outlet
    out, clo = ft.outlets_and_closure(ip, ix, sg, np.array([1, 2]))
    assert out.tolist() == [2] and clo.tolist() == [1, 2]       # A is not upstream of B through UM


def test_local_csr_keeps_the_stored_order_and_the_tables():
    um = _graph(6, [(0, 1), (1, 2), (3, 2), (5, 3)])
    basin_ids = np.array([1, 1, 1, 1, 2, 3])
    L, V, A, S0 = np.arange(1.0, 7.0) * 1000, np.full(6, 0.5), np.arange(6) + 10.0, np.arange(6) * 100.0
    t = ft.FlowTables(um, basin_ids, [1, 3], L, V, A, S0, np.full(12, 30), 12, 3)
    assert t.closures[0].tolist() == [0, 1, 2, 3, 5] and t.closures[1].tolist() == [5]
    assert t.closure_ptr.tolist() == [0, 5, 6]
    c = t.closures[0]
    sub = um[c][:, c].tocsr()
    assert np.array_equal(t.row_ptr[:6], sub.indptr)
    assert np.array_equal(t.cols[:sub.nnz], sub.indices) and np.array_equal(t.sign[:sub.nnz], sub.data)
    assert t.basin_col.tolist() == [0, 1, 2, 3, -1, 0]
    assert t.outlet_rank.tolist() == [-1, -1, 0, -1, -1, 0]
    assert np.array_equal(t.tauinv, (V / L)[[0, 1, 2, 3, 5, 5]])
    assert np.array_equal(t.s0, S0[[0, 1, 2, 3, 5, 5]])
    assert t.weights.tolist() == [5 * 15, 1 * 15]
    j = ft.FlowTables.join([t.part(1), t.part(0)])
    assert j.basins == [3, 1] and j.closure_ptr.tolist() == [0, 1, 6]
    assert np.array_equal(j.cols, np.concatenate([t.cols[sub.nnz:], t.cols[:sub.nnz]]))
    assert j.row_ptr.tolist() == [0, 1] + (t.row_ptr[1:6] + 1).tolist()


def test_closure_matches_the_world_route(golden):
    """Routing the closure alone gives the outlet series of routing the world (oracle loops, bit for bit)."""
    from oracle import mrtm as o_mrtm
    g = golden('flowcal')
    um = _um(g)
    nm, rspin = int(g['nmonths']), int(g['routing_spinup'])
    t = ft.FlowTables(um, g['basin_ids'], [3], g['flow_dist'], g['velocity'], g['area'], g['chs_prev'], g['ndays'], nm,
                      rspin)
    rng = np.random.default_rng(3)
    q = np.zeros((um.shape[0], nm))
    q[g['basin_ids'] == 3] = rng.uniform(0, 50, ((g['basin_ids'] == 3).sum(), nm))
    _, avg, _ = o_mrtm.route_series(um, g['flow_dist'], g['velocity'], g['area'], q, g['ndays'], rspin,
                                    S0=g['chs_prev'])
    sub = sparse.csr_matrix((t.sign.astype(int), t.cols, t.row_ptr), shape=(t.closures[0].size,) * 2)
    c = t.closures[0]
    _, avg_c, _ = o_mrtm.route_series(sub, g['flow_dist'][c], g['velocity'][c], g['area'][c], q[c], g['ndays'], rspin,
                                      S0=g['chs_prev'][c])
    assert np.array_equal(avg_c, avg[c])


def test_refusals(tmp_path):
    s = NS(pet_module='none', runoff_module='abcd', routing_module='none', calibrate=1, set_calibrate=1)
    with pytest.raises(ValidationException, match='routing_module = mrtm'):
        check_modules(s)
    s.routing_module = 'mrtm'
    check_modules(s)
    # ... and when the ini is read: a synthetic tree with set_calibrate = 1, once with MRTM and once without
    from xanthos_amd import synth
    from xanthos_amd.ini_reader import ConfigReader
    w = synth.make_world(nrow=12, ncol=24, ncell=120, n_basins=3, seed=2)
    f = synth.make_forcing(w, 36)
    obs = np.stack([np.ones(36), np.zeros(36), np.zeros(36), np.arange(36) + 1.0], 1)
    ini = synth.write_example(str(tmp_path), w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, obs=obs,
                              set_calibrate=1)
    c = ConfigReader(ini)
    assert c.set_calibrate == 1 and c.obs_unit == 'm3_per_sec'
    text = open(ini).read()
    assert 'routing_module = mrtm' in text
    open(ini, 'w').write(text.replace('routing_module = mrtm', 'routing_module = none'))
    with pytest.raises(ValidationException, match='set_calibrate = 1.*routing_module = mrtm'):
        ConfigReader(ini)
    # NaN forcing: every affected basin and its first such cell
    pr = np.ones((6, 30))
    pr[4, 7] = np.nan
    pet = np.ones((6, 30))
    pet[5, 29] = np.nan
    with pytest.raises(ValidationException, match=r'basin 2 \(cell 4\).*basin 3 \(cell 5\)'):
        ft.check_forcing([1, 2, 3], np.array([1, 1, 1, 1, 2, 3]), pet, pr, 30)
    ft.check_forcing([1], np.array([1, 1, 1, 1, 2, 3]), pet, pr, 30)
    # a closure larger than the kernel takes
    n = 40
    um = _graph(n, [(i, i + 1) for i in range(n - 1)])
    with pytest.raises(ValidationException, match='basin 1 has 40 cells.*at most 32'):
        ft.FlowTables(um, np.ones(n, dtype=int), [1], np.ones(n), np.ones(n), np.ones(n), None, np.full(12, 30), 12, 0,
                      max_closure=32)


def test_calibrate_accepts_set_calibrate_1_until_the_device():
    """set_calibrate = 1 is accepted and its tables built; without a GPU the search raises HipUnavailable (no fallback)."""
    from xanthos_amd import _hip
    um = _graph(6, [(0, 1), (1, 2), (3, 2), (5, 3)])
    nm = 30
    data = NS(basin_ids=np.array([1, 1, 1, 1, 2, 3]), area=np.ones(6), precip=np.ones((6, nm)), tmin=None,
              cal_obs=np.stack([np.ones(nm), np.arange(nm) + 1.0], 1), flow_dist=np.full(6, 1e4),
              str_velocity=np.ones(6), chs_prev=np.zeros(6))
    settings = NS(set_calibrate=1, obs_unit='m3_per_sec', cal_basins=['1'], nmonths=nm, runoff_spinup=25,
                  routing_spinup=3, calib_out_dir=None, device=0)
    with pytest.raises(ValueError, match='um'):
        calibrate_all(settings, data, np.ones((6, nm)))
    if _hip.device_count() > 0:
        return
    with pytest.raises(_hip.HipUnavailable):
        calibrate_all(settings, data, np.ones((6, nm)), um=um, ndays=np.full(nm, 30))
    with pytest.raises(_hip.HipUnavailable):
        Calibrate(basin_num=1, basin_ids=data.basin_ids, basin_areas=data.area, precip=data.precip,
                  pet=np.ones((6, nm)), obs=data.cal_obs, tmin=None, n_months=nm, runoff_spinup=25, set_calibrate=1,
                  obs_unit='m3_per_sec', out_dir=None, um=um, flow_dist=data.flow_dist, velocity=data.str_velocity,
                  ndays=np.full(nm, 30), routing_spinup=3).calibrate_basin()
