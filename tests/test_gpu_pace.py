"""GPU tests (-m gpu) of the pair shapes of the reassociated routing kernel that know their outlet rounds at compile time
(NXR in xanthos_amd/csrc/xh_mrtm_wave_unit.h, instantiated in xh_mrtm_rsum.hip).

Reference: xanthos/routing/mrtm.py:50-69 through the oracle.  A prepared plan passes one running sum per lane; the cells that may
fire and have an upstream neighbour that may sit in pair units, and what their EXIT lanes send to single units is guarded
(>= -1e-10 m3/s in every sub-step; a trip routes the call again on the plan of pairs).  Every pair unit now runs a shape built
for "no outlet" or "one round of outlets": the outlet's LDS read, its store, the store of the run's last block and the guard are
the code these tests walk.  The bar is the form's: identical NaN masks and |x - ref| <= 1e-9 |ref| + atol, atol 1e-3 m3 for
storages and 1e-9 m3/s for flows (tests/test_gpu_reassoc.py).  Every case runs in a child process: the switches are read when
the library builds its plan.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

_CORNER_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import corner_world as cw
from oracle import mrtm as o_mrtm
from xanthos_amd import _hip
from xanthos_amd.routing import mrtm
seed, mode, ndays, spin = int(sys.argv[2]), sys.argv[3], np.array(json.loads(sys.argv[4])), int(sys.argv[5])
idx, csr, L, v, area = cw.make(seed=seed)
n = len(L)
q = cw.runoff(n, nmonths=6, seed=seed)                # the six months the seeds were picked for ...
if len(ndays) > 6:                                    # ... and more of the same behind them
    q = np.concatenate([q, cw.runoff(n, nmonths=len(ndays) - 6, seed=seed + 1000)], axis=1)
if mode == 'negative_runoff':
    q[idx['s0_t1_0'], 3] = -5.0                       # outside the argument (lateral inflow >= 0): the guard must trip
um = mrtm.UpstreamMatrix(*csr)
fired, neg_s, neg_f = cw.instrumented(csr, L, v, area, q[:, :6], ndays[:6])
ref = o_mrtm.route_series(um.tocsr(), L, v, area, q, ndays, spin)
got = mrtm.route_series(um, L, v, area, q, ndays, spin)
plan = um.plan(_hip.get_context())
worst = 0.0
for x, r, atol in zip(got, ref, (1e-3, 1e-9, 1e-9)):
    assert np.array_equal(np.isnan(x), np.isnan(r))
    err = np.abs(x - r)
    print('largest excess over the bar', float((err - (1e-9 * np.abs(r) + atol)).max()), file=sys.stderr)
    assert (err <= 1e-9 * np.abs(r) + atol).all(), float((err - 1e-9 * np.abs(r)).max())
    worst = max(worst, float((err / np.maximum(np.abs(r), 1e6 * atol)).max()))
info = plan.info()
print(json.dumps({'kernel': int(info['last_tree_kernel']), 'rsum': plan.rsum_info(), 'worst': worst, 'reroutes': int(info['reroutes']),
                  'guard_trips': int(plan.rsum_info()['guard_trips']), 'neg_storage_cells': int((neg_s > 0).sum()),
                  'neg_flow_at_A': [int(neg_f[idx['s%d_A' % k]]) for k in range(3)]}))
"""

_WORLD_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import mrtm as o_mrtm
from xanthos_amd import _hip, synth
from xanthos_amd.pipeline import pipeline_from_world
ctx = _hip.get_context(0)
w = synth.make_world(nrow=60, ncol=120, ncell=3000, n_basins=5, seed=3, outlet_frac=0.02)      # _world() of test_gpu_reassoc.py
nm, spin = 36, 12      # (ABCD's own spin-up is 25 months at the least and has to fit into the run: 36 months, not 24)
pipe = pipeline_from_world(ctx, w, nm, 1971, 25, spin)       # (makes the prepared plan: velocity, flow distance, dt)
ctx.synth_forcing(7, w.ncell, nm, ctx.upload(w.latitude), pipe.alloc_forcing(), nan_frac=0.003)
out = {}
ref = None
for order, fed in (('staged', False), ('fed', True)):
    for k in ('chs', 'avg'):
        pipe.out[k].zero()
    pipe.run(fed=fed)
    ctx.sync()
    if ref is None:
        ref = o_mrtm.route_series(pipe.um.tocsr(), w.flow_dist, w.velocity, w.area, pipe.out['q'].download(), pipe.ndays, spin)
    worst = 0.0
    for k, r, atol in (('chs', ref[0], 1e-3), ('avg', ref[1], 1e-9)):
        x = pipe.out[k].download()
        assert np.array_equal(np.isnan(x), np.isnan(r)), (order, k)
        m = ~np.isnan(r)
        err = np.abs(x[m] - r[m])
        print(order, k, 'largest excess over the bar', float((err - (1e-9 * np.abs(r[m]) + atol)).max()), file=sys.stderr)
        assert (err <= 1e-9 * np.abs(r[m]) + atol).all(), (order, k, float(err.max()))
        worst = max(worst, float((err / np.maximum(np.abs(r[m]), 1e6 * atol)).max()))
    out[order] = {'worst': worst, 'kernel': int(pipe.plan.info()['last_tree_kernel']), 'rsum': pipe.plan.rsum_info()}
print(json.dumps(out))
"""

SIX = [31, 28, 31, 30, 31, 30]
TWO_YEARS = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31] * 2
# 13 months that end in a 28-day February: an odd number of months, 3,144 sub-steps = 196.5 groups of 16 -- whatever a unit's lag,
# its run ends inside a group, and the last outlet block is the one stored after the loops
THIRTEEN = SIX + [31, 31, 30, 31, 30, 31, 28]


def _child(tmp_path, text, args, env=None):
    script = tmp_path / 'pace_child.py'
    script.write_text(text)
    e = dict(os.environ, XH_FLOW_CHECK='1')
    e.pop('XH_ROUTE_REASSOC', None)
    e.update(env or {})
    r = subprocess.run([sys.executable, str(script), ROOT] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stderr[-600:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize('seed', [3, 13, 20])
def test_corner_world_two_years_on_the_prepared_plan(tmp_path, seed):
    """The corner S1 >= 0 > S2 of mrtm.py:54, :66-69 (tests/corner_world.py) for 24 months behind a 12-month spin-up: routed by the
    reassociated kernel on the single-sum plan, within the bar of the oracle, no guard tripped."""
    out = _child(tmp_path, _CORNER_CHILD, [seed, 'plain', json.dumps(TWO_YEARS), 12])
    assert out['neg_storage_cells'] >= 1, out                                   # the corner does occur
    assert out['kernel'] == 4, out
    assert out['rsum']['pair_cells'] > 0 and out['rsum']['pair_units'] >= 1, out
    assert out['rsum']['fold_disabled'] == 0 and out['guard_trips'] == 0 and out['reroutes'] == 0, out


def test_synthetic_world_three_years_staged_and_fed(tmp_path):
    """3,000 cells (networks far larger than a unit: streams, outlets and imports in most units), 36 months behind a routing spin-up
    of 12 (three years, not two: the pipeline's ABCD stage needs 25 months of spin-up inside the run), the stage-by-stage and the
    fed order: both within the bar of the oracle routing of the same runoff, on the prepared plan.  No cell of this world needs
    the pair form (pair_cells 0): its units are single units, whose shapes keep the run-time outlet rounds -- this is the check
    that they route as before beside the new pair shapes; the pair shapes themselves run in the corner worlds of this file."""
    out = _child(tmp_path, _WORLD_CHILD, [])
    print(out)
    for order in ('staged', 'fed'):
        o = out[order]
        assert o['kernel'] == 4, out
        assert o['rsum']['pair_cells'] == 0, out                    # (a world with cells in pair form would be another test)
        assert o['rsum']['fold_disabled'] == 0 and o['rsum']['guard_trips'] == 0, out


def test_exit_guard_trips_and_the_call_is_rerouted(tmp_path):
    """The inputs of test_single_sum_guards_trip_and_the_call_is_rerouted (tests/test_gpu_reassoc.py) through the pair shapes with
    compile-time outlet rounds: (a) no halo -- the corner cell's negative outflow leaves the pair units through an exit lane and
    trips the exit guard; (b) negative runoff trips the runoff guard.  Either way: routed again on the plan of pairs, within the
    bar."""
    a = _child(tmp_path, _CORNER_CHILD, [3, 'plain', json.dumps(SIX), 0], {'XH_RSUM_HALO': '0'})
    assert sum(a['neg_flow_at_A']) > 0, a                                        # the reference does send negative flow out of A
    assert a['kernel'] == 4, a
    assert a['rsum']['fold_disabled'] == 1 and a['rsum']['pair_cells'] == -1 and a['guard_trips'] >= 1, a
    b = _child(tmp_path, _CORNER_CHILD, [3, 'negative_runoff', json.dumps(SIX), 0])
    assert b['kernel'] == 4, b
    assert b['rsum']['fold_disabled'] == 1 and b['rsum']['pair_cells'] == -1 and b['guard_trips'] >= 1, b


def test_run_that_ends_inside_a_group(tmp_path):
    """13 months ending in a 28-day February, no spin-up (THIRTEEN above): every unit's run ends inside a group of 16 sub-steps,
    and the last outlet block is the partial one stored after the loops -- by the shapes with one compile-time round of outlets
    here.  Within the bar, nothing trips."""
    out = _child(tmp_path, _CORNER_CHILD, [3, 'plain', json.dumps(THIRTEEN), 0])
    assert out['kernel'] == 4, out
    assert out['rsum']['pair_cells'] > 0 and out['rsum']['pair_units'] >= 1, out
    assert out['guard_trips'] == 0 and out['rsum']['fold_disabled'] == 0, out
