"""GPU tests (-m gpu) of the once-a-month path of the time-skewed routing kernels (xanthos_amd/csrc/xh_mrtm_wave_unit.h): the
month bookkeeping that sits between the runs of groups, the 64-byte month records it reads a month ahead (xh_mrtm_rec.h: the
lanes' next crossing, the reciprocals the reassociated kernel multiplies by) and the output groups of four months.

Reference: xanthos/routing/mrtm.py:16-82 and components.py:273-294 through the oracle (oracle/mrtm.py).  The bar is the
reassociated form's (tests/test_gpu_reassoc.py, routed_close): identical NaN masks and |x - ref| <= 1e-9 |ref| + atol, atol
1e-3 m3 for storages and 1e-9 m3/s for flows.  Every case runs in a child process of its own, under a time limit: the switches
are read when the library builds its plan.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

_PRELUDE = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import corner_world as cw
from oracle import mrtm as o_mrtm
from xanthos_amd import _hip
from xanthos_amd.routing import mrtm


def close(got, ref, tag):
    worst = 0.0
    for x, r, atol, name in zip(got, ref, (1e-3, 1e-9, 1e-9), ('chs', 'avg', 'F_end')):
        assert x.shape == r.shape, (tag, name)
        assert np.array_equal(np.isnan(x), np.isnan(r)), ('NaN pattern differs', tag, name)
        m = ~np.isnan(r)
        excess = np.abs(x[m] - r[m]) - (atol + 1e-9 * np.abs(r[m]))
        print(tag, name, 'largest excess over the bar', float(excess.max()) if m.any() else None, file=sys.stderr)
        assert (excess <= 0).all(), (tag, name, int((excess > 0).sum()), float(excess.max()))
        if m.any():
            worst = max(worst, float(np.max(np.abs(x[m] - r[m]) / np.maximum(np.abs(r[m]), atol * 1e6))))
    return worst
"""

# January 1960 onwards: 31, 29 (a leap year), 31, 30, ... and February 1961 as the 14th month -- 248, 232, 240 and 224 sub-steps
FROM_1960 = [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31, 31, 28]

_RECORDS_CHILD = _PRELUDE + r"""
nmonths, dt = int(sys.argv[2]), float(sys.argv[3])
ndays = np.array(json.loads(sys.argv[4]))[:nmonths]
idx, csr, L, v, area = cw.make(seed=3, dt=dt)
n = len(L)
q = cw.runoff(n, nmonths=max(nmonths, 6), seed=3)[:, :nmonths].copy()
q[idx['s1_t0_0'], min(1, nmonths - 1)] = np.nan           # one cell without runoff data in one month: NaN from there on, downstream too
um = mrtm.UpstreamMatrix(*csr)
out = {'cases': []}
for spin in (0, 1, 5):
    if spin > nmonths:
        continue
    ref = o_mrtm.route_series(um.tocsr(), L, v, area, q, ndays, spin, dt=dt)
    got = mrtm.route_series(um, L, v, area, q, ndays, spin, dt=dt)
    assert np.isnan(ref[0]).any()
    worst = close(got, ref, 'months %d spin-up %d' % (nmonths, spin))
    plan = um.plan(_hip.get_context())
    out['cases'].append({'spin': spin, 'worst': worst, 'kernel': int(plan.info()['last_tree_kernel']), 'rsum': plan.rsum_info()})
print(json.dumps(out))
"""

_FOLD_CHILD = _PRELUDE + r"""
rng = np.random.default_rng(11)
dt = 10800.0
sizes = rng.integers(3, 7, 60)                          # 60 star networks: an outlet and 2 - 5 leaves that drain into it
n = int(sizes.sum())
down = np.full(n, -1)
leaves, at = [], 0
for s in sizes:                                         # the outlet in the middle of its star's ids: as on a D8 grid, a row has at most
    centre = at + (s - 1) // 2                          # four terms either side of its diagonal
    for c in range(at, at + s):
        if c != centre:
            down[c] = centre
            leaves.append(c)
    at += s
rows = [[(i, -1)] for i in range(n)]
for c in range(n):
    if down[c] >= 0:
        rows[down[c]].append((c, 1))
indptr, indices, data = [0], [], []
for r in rows:
    for col, sg in sorted(r):
        indices.append(col)
        data.append(sg)
    indptr.append(len(indices))
v = np.full(n, 1.0)
L = np.full(n, dt / 0.27)
ratio = np.logspace(-5, np.log10(0.99), len(leaves))    # velocity * dt / length of the leaves: none of them can fire
L[leaves] = dt * v[leaves] / rng.permutation(ratio)
area = rng.uniform(2450.0, 2550.0, n)
nmonths = 24
ndays = np.array(([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31] * 2)[:nmonths])
q = rng.gamma(2.0, 30.0, (n, nmonths))
q[:, 7] *= 0.02                                         # a dry month
q[leaves[5], :] = 0.0                                   # a leaf without any runoff
S0 = rng.uniform(0.0, 5e6, n)
S0[leaves[9]] = 0.0
um = mrtm.UpstreamMatrix(np.array(indptr), np.array(indices), np.array(data))
ref = o_mrtm.route_series(um.tocsr(), L, v, area, q, ndays, 0, S0=S0, dt=dt)
got = mrtm.route_series(um, L, v, area, q, ndays, 0, S0=S0, dt=dt)
worst = close(got, ref, 'stars, 24 months')
plan = um.plan(_hip.get_context())
info = {'kernel': int(plan.info()['last_tree_kernel']), 'rsum': plan.rsum_info(), 'cells': n}
# one month through streamrouting, which takes the initial storage as the reference's does
ref1 = o_mrtm.streamrouting(L, S0, np.zeros(n), v, q[:, 0], area, 31, dt, um.tocsr())
got1 = mrtm.streamrouting(L, S0, np.zeros(n), v, q[:, 0], area, 31, dt, um)
worst = max(worst, close(got1, ref1, 'stars, one month'))
info['kernel_one_month'] = int(plan.info()['last_tree_kernel'])
info['worst'] = worst
print(json.dumps(info))
"""

_CONTINUITY_CHILD = _PRELUDE + r"""
dt = 10800.0
ndays = np.array(json.loads(sys.argv[2]))
idx, csr, L, v, area = cw.make(seed=3, dt=dt)
n = len(L)
q = cw.runoff(n, nmonths=6, seed=3)
um = mrtm.UpstreamMatrix(*csr)
ref = o_mrtm.route_series(um.tocsr(), L, v, area, q, ndays, 0, dt=dt)
whole = mrtm.route_series(um, L, v, area, q, ndays, 0, dt=dt)
a = mrtm.route_series(um, L, v, area, q[:, :3].copy(), ndays[:3], 0, dt=dt)
b = mrtm.route_series(um, L, v, area, q[:, 3:].copy(), ndays[3:], 0, S0=a[0][:, -1].copy(), dt=dt)      # (F is recomputed: mrtm.py:50)
chained = (np.concatenate([a[0], b[0]], axis=1), np.concatenate([a[1], b[1]], axis=1), b[2])
worst = max(close(whole, ref, 'six months'), close(chained, ref, 'three and three months'))
plan = um.plan(_hip.get_context())
print(json.dumps({'worst': worst, 'kernel': int(plan.info()['last_tree_kernel']), 'rsum': plan.rsum_info(),
                  'bit_equal': bool(all(np.array_equal(x, y, equal_nan=True) for x, y in zip(whole, chained)))}))
"""


def _child(tmp_path, text, args):
    script = tmp_path / 'month_path_child.py'
    script.write_text(text)
    e = dict(os.environ, XH_FLOW_CHECK='1')
    e.pop('XH_ROUTE_REASSOC', None)
    r = subprocess.run([sys.executable, str(script), ROOT] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stderr[-900:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize('nmonths', [1, 2, 3, 5, 13, 14])
def test_records_and_output_groups(tmp_path, nmonths):
    """The corner world (tests/corner_world.py, ~100 cells, prepared plan) from January 1960, so that months of 224, 232, 240 and
    248 sub-steps occur; series of 1, 2, 3, 5, 13 and 14 months -- the edges `it + 1 < nit` and `it + 2 < nit` of the month
    bookkeeping, last output groups of 1, 2 and 4 months -- each behind routing spin-ups of 0, 1 and 5 months (those that fit
    into the series), so that the write flag starts at every position of an output group; one cell has NaN runoff in one
    month, and the NaN mask must be the oracle's.  Within the form's bar, routed by the reassociated dataflow kernel."""
    out = _child(tmp_path, _RECORDS_CHILD, [nmonths, 10800.0, json.dumps(FROM_1960)])
    print(out)
    assert [c['spin'] for c in out['cases']] == [s for s in (0, 1, 5) if s <= nmonths], out
    for c in out['cases']:
        assert c['kernel'] == 4, out


def test_odd_sub_step_counts(tmp_path):
    """The same world at dt = 17,280 s (five sub-steps a day: months of 155, 145 and 155 sub-steps) for three months: lanes cross
    a month start at odd iterations too -- the boundary loop that is not the mid-zone copy, and its `odd_ok` crossings."""
    out = _child(tmp_path, _RECORDS_CHILD, [3, 17280.0, json.dumps(FROM_1960)])
    print(out)
    for c in out['cases']:
        assert c['kernel'] == 4, out


def test_folded_leaves(tmp_path):
    """60 star networks of 3 - 6 cells without any stream between units, the leaves' velocity * dt / length spread
    logarithmically over 1e-5 .. 0.99, one leaf without runoff, one dry month, 24 months from a non-zero initial storage (and one
    month through streamrouting): leaves ride in their parents' lanes, their month bookkeeping on the carriers'."""
    out = _child(tmp_path, _FOLD_CHILD, [])
    print(out)
    assert 200 <= out['cells'] <= 360, out
    assert out['kernel'] == 4 and out['kernel_one_month'] == 4, out
    assert out['rsum']['folded'] > 0 and out['rsum']['fold_disabled'] == 0 and out['rsum']['guard_trips'] == 0, out


def test_continuity_of_chained_calls(tmp_path):
    """Six months in one call against three and three months chained through the end storage: both within the form's bar of
    the oracle's six months.  Whether the two are bit-equal is printed, not asserted (the first month of a call takes its
    lateral inflow in the prologue, the later ones from the records: the same factor, formed the same way)."""
    out = _child(tmp_path, _CONTINUITY_CHILD, [json.dumps(FROM_1960[:6])])
    print(out)
    print('one call and the chained calls bit-equal:', out['bit_equal'])
    assert out['kernel'] == 4, out
