"""GPU tests (-m gpu) of the flow-control checks of the two dataflow routing kernels (check() in
xanthos_amd/csrc/xh_mrtm_wave_unit.h, the rule in xh_mrtm_flowctl.h): a unit asks for a stream counter only when the value it
last saw does not cover what its next 256 sub-steps need, and publishes at every check as before.

Reference: xanthos/routing/mrtm.py through the oracle.  For every case the bit-exact kernel (k_mrtm_wave, XH_ROUTE_EXACT) must
equal the oracle bit for bit and the default kernel (k_mrtm_rsum) must meet the bars of tests/test_gpu_reassoc.py: identical NaN
masks and |x - ref| <= 1e-9 |ref| + atol, atol 1e-3 m3 for storages and 1e-9 m3/s for flows.  A dataflow kernel must really
have run (last_tree_kernel 2 or 4), no guard may trip and no call may be routed again: every wait in the kernels is bounded
at 5 s and a timeout raises the fault word, which routes the call again and is counted (`reroutes`) -- a flow-control bug shows
there or as a wrong value, not as a hang.  The fault word itself is not readable from Python: a word left set would make the
next dataflow launch give up at once, so each case routes twice (both kernels) and both must come through a dataflow kernel with
`reroutes` still 0.

Worlds: tests/corner_world.py (cells that can fire, halos, pair units) and the most chain-heavy tree the generators of
tests/test_gpu_linear_units.py make: random_tree with reach 1, ONE river of 450 cells (ids shuffled), a fifth of whose cells can
fire, cut into pieces of at most 8 cells (XH_FLOW_PIECE_CAP): some 60 units, each importing from the one above it, a chain of
streams as deep as there are units.  No tributaries on purpose: a stream that jumps over k pipeline levels needs a ring of
1,024 + 768 k sub-steps (xh_mrtm_wave_launch.hip), so with the smallest ring the launch accepts -- 2,048 -- a tributary that joins
a deep stem starves until a bounded wait gives up (tests/test_gpu_reassoc.py has that case); a river without tributaries has no
such stream and the smallest ring is a legal one for it.  36 months behind a spin-up of 12 at dt 3 h are 11,680
sub-steps = 45 checks; with the smallest legal ring (XH_FLOW_RS=2048, 8 check intervals) a producer has to look at `done` again
and again while a consumer behind a fast producer runs on one look for many checks, and the per-unit accounting
(XH_FLOW_STATS=1: bits 36-49 / 50-63 of words 4 and 5, tools/rsum_probe.py) must show both.  Every case is a child process: the
switches are read when the library builds its plan.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import corner_world as cw
from test_gpu_linear_units import csr_of, random_tree, shuffled
from oracle import months as o_months
from oracle import mrtm as o_mrtm
from xanthos_amd import _hip
from xanthos_amd.routing import mrtm
world, ndays, spin = sys.argv[2], np.array(json.loads(sys.argv[3])), int(sys.argv[4])
if world == 'corner':
    idx, csr, L, v, area = cw.make(seed=3)
    n = len(L)
    q = cw.runoff(n, nmonths=6, seed=3)
    if len(ndays) > 6:
        q = np.concatenate([q] + [cw.runoff(n, nmonths=6, seed=1000 + k) for k in range((len(ndays) - 1) // 6)], axis=1)
    q = q[:, :len(ndays)]
else:
    rng = np.random.default_rng(41)
    n = 450
    ds, _ = shuffled(rng, random_tree(rng, n, reach=1, fan=1))      # one river, no tributary: every stream joins adjacent levels
    csr = csr_of(ds)
    L = np.full(n, 40e3)
    v = np.where(rng.random(n) < 0.2, 5.0, 1.0)                     # velocity * dt / length 1.35 (may fire) or 0.27
    area = rng.uniform(2450.0, 2550.0, n)
    q = rng.gamma(2.0, 30.0, (n, len(ndays)))
    q[:, len(ndays) // 2] *= 0.02                                   # a dry month
um = mrtm.UpstreamMatrix(*csr)
ctx = _hip.get_context()
ref = o_mrtm.route_series(um.tocsr(), L, v, area, q, ndays, spin)
out = {}


def looks(plan):
    st = plan.stats()
    if st is None:
        return None
    f = lambda k, sh: int(((st[:, k] >> np.uint64(sh)) & np.uint64(0x3fff)).sum())
    return {'ready_looked': f(4, 36), 'ready_covered': f(4, 50), 'done_looked': f(5, 36), 'done_covered': f(5, 50), 'units': int(len(st))}


for name, flags in (('exact', _hip.XH_ROUTE_EXACT), ('rsum', 0)):
    got = mrtm.route_series(um, L, v, area, q, ndays, spin, flags=flags)
    ctx.sync()
    plan = um.plan(ctx)
    info = plan.info()
    o = {'kernel': int(info['last_tree_kernel']), 'reroutes': int(info['reroutes']), 'units': int(info['flow_units']),
         'edges': int(info['flow_edges']), 'depth': int(info['flow_depth']), 'rsum': plan.rsum_info(), 'looks': looks(plan)}
    if name == 'exact':
        o['bit_identical'] = bool(all(np.array_equal(x, r, equal_nan=True) for x, r in zip(got, ref)))
    else:
        o['nan_equal'] = bool(all(np.array_equal(np.isnan(x), np.isnan(r)) for x, r in zip(got, ref)))
        worst = -np.inf
        for x, r, atol in zip(got, ref, (1e-3, 1e-9, 1e-9)):
            m = ~np.isnan(r) & ~np.isnan(x)
            if m.any():
                worst = max(worst, float((np.abs(x[m] - r[m]) - (1e-9 * np.abs(r[m]) + atol)).max()))
        o['largest_excess_over_the_bar'] = worst
    print(name, o, file=sys.stderr)
    out[name] = o
out['sub_steps'] = int((ndays.sum() + ndays[:spin].sum()) * 8)
print(json.dumps(out))
"""

THREE_YEARS = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31] * 3
SIX = [31, 28, 31, 30, 31, 30]
SMALL = {'XH_FLOW_PIECE_CAP': '8', 'XH_FLOW_RS': '2048'}


def _run(tmp_path, world, ndays, spin, env):
    script = tmp_path / 'check_path_child.py'
    script.write_text(_CHILD)
    e = dict(os.environ, XH_FLOW_CHECK='1', XH_FLOW_STATS='1')
    for k in ('XH_ROUTE_REASSOC', 'XH_FLOW_LOOK_ALWAYS', 'XH_ROUTE_FENCED'):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, str(script), ROOT, world, json.dumps(ndays), str(spin)], env=e, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for name in ('exact', 'rsum'):
        o = out[name]
        assert o['kernel'] in (2, 4), (name, o)                       # the dataflow kernel really ran ...
        assert o['reroutes'] == 0, (name, o)                          # ... no bounded wait gave up, the fault word stayed clear
        assert o['rsum']['guard_trips'] == 0, (name, o)
    assert out['exact']['bit_identical'], out['exact']
    assert out['rsum']['nan_equal'] and out['rsum']['largest_excess_over_the_bar'] <= 0.0, out['rsum']
    return out


def test_corner_world_both_kernels(tmp_path):
    out = _run(tmp_path, 'corner', SIX, 0, {})
    assert out['rsum']['rsum']['pair_units'] >= 1, out


def test_one_river_small_pieces_small_rings_looks_and_skips(tmp_path):
    """Both branches of the rule within one run, for both counters and both kernels: with rings of 8 check intervals a producer's
    known `done` runs out every few checks (it looks), and between those checks it is covered (it does not)."""
    out = _run(tmp_path, 'tree', THREE_YEARS, 12, SMALL)
    assert out['sub_steps'] == 11680 and out['rsum']['units'] >= 30 and out['rsum']['edges'] >= 29 and out['rsum']['depth'] >= 3, out
    for name in ('exact', 'rsum'):
        lk = out[name]['looks']
        assert lk is not None, out
        assert lk['ready_looked'] > 0 and lk['ready_covered'] > 0 and lk['done_looked'] > 0 and lk['done_covered'] > 0, (name, lk)


def test_fewer_sub_steps_than_two_check_intervals(tmp_path):
    out = _run(tmp_path, 'tree', [31, 28], 0, SMALL)
    assert out['sub_steps'] == 472 and out['rsum']['edges'] >= 29, out


def test_linear_units_clamping(tmp_path):
    out = _run(tmp_path, 'tree', SIX, 2, dict(SMALL, XH_RSUM_LINEAR='0'))
    assert out['rsum']['rsum']['linear_units'] == 0, out


def test_without_folded_leaves(tmp_path):
    out = _run(tmp_path, 'tree', SIX, 2, dict(SMALL, XH_FLOW_FOLD='0'))
    assert out['rsum']['rsum']['folded'] == 0, out
