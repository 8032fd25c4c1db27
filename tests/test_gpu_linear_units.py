"""GPU tests (-m gpu) of the LINEAR single units of the reassociated routing kernel (LIN in xanthos_amd/csrc/xh_mrtm_wave_unit.h,
unit_p bit 5 of xh_flow_rsum.cpp) and of the single shapes that know their outlet rounds at compile time (NXR).

Reference: xanthos/routing/mrtm.py:50-69 through the oracle.  A single unit none of whose cells may fire (velocity * dt / length
below 1 and outside every halo) never takes the branch of mrtm.py:54, so its step is the recurrence
S <- (sum F2) dt + (S a + erl dt), outflow S / tau, and the month's mean flow is (sum S) / tau / nt: results move by roundings only.
The bar is the form's own: identical NaN masks and |x - ref| <= 1e-9 |ref| + atol, atol 1e-3 m3 for storages, 1e-9 m3/s for flows
(tests/test_gpu_reassoc.py).  Every case routes 4 months of 3-hour sub-steps (960: three check() intervals of 256, three month
crossings) through routing.mrtm.route_series, which prepares the plan for the call's velocity, flow distance and dt.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FOUR = np.array([31, 28, 31, 30])
DT = 10800.0
BAR = (1e-3, 1e-9, 1e-9)                       # ChStorage (m3), Avg_ChFlow (m3/s), F_end (m3/s)


def csr_of(ds):
    """UM = UP - I as CSR arrays (mrtm.py:194-230) of a forest given by every cell's downstream cell (-1: an outlet)."""
    n = len(ds)
    rows = [[(i, -1)] for i in range(n)]
    for c, d in enumerate(ds):
        if d >= 0:
            rows[d].append((c, 1))
    indptr, indices, data = [0], [], []
    for r in rows:
        for col, sg in sorted(r):
            indices.append(col)
            data.append(sg)
        indptr.append(len(indices))
    return np.array(indptr), np.array(indices), np.array(data)


def random_tree(rng, n, reach=12, fan=3):
    """ds[] of one network of n cells: cell 0 is the outlet, every other cell drains to one of the `reach` cells in front of it
    that has fewer than `fan` upstream neighbours so far."""
    ds = np.full(n, -1)
    deg = np.zeros(n, int)
    for i in range(1, n):
        cand = [j for j in range(max(0, i - reach), i) if deg[j] < fan]
        ds[i] = cand[rng.integers(len(cand))] if cand else i - 1
        deg[ds[i]] += 1
    return ds


def shuffled(rng, ds):
    """The same forest with its cell ids permuted (the planner must not depend on a topological numbering)."""
    n = len(ds)
    perm = rng.permutation(n)
    out = np.full(n, -1)
    for c in range(n):
        out[perm[c]] = perm[ds[c]] if ds[c] >= 0 else -1
    return out, perm


def quiet_world(seed=1, n=320):
    """(a) A few hundred cells in ONE network, velocity * dt / length = 0.27 everywhere: no cell may fire."""
    rng = np.random.default_rng(seed)
    ds, _ = shuffled(rng, random_tree(rng, n))
    return ds, np.full(n, 40e3), np.full(n, 1.0), rng.uniform(2450.0, 2550.0, n)


def comb_world(seed=2, stem=13, n_trib=12, trib=64):
    """(c) A stem of `stem` cells with a tributary of `trib` cells (a full unit: it is cut off and arrives as a stream) at each
    of `n_trib` stem cells: the unit of the stem imports 12 streams (two import rounds, NG = 2) and has no outlet, each
    tributary's unit has one outlet and no import (the host planner on this topology: 13 units, 12 streams, one unit with
    more than 8 imports).  Nothing can fire."""
    rng = np.random.default_rng(seed)
    ds = [-1] + list(range(stem - 1))                       # stem: cell k drains to k - 1
    for t in range(n_trib):
        base = len(ds)
        sub = random_tree(rng, trib)
        ds += [t + 1 if d < 0 else base + d for d in sub]
    ds, perm = shuffled(rng, np.array(ds))
    n = len(ds)
    return ds, np.full(n, 40e3), np.full(n, 1.0), rng.uniform(2450.0, 2550.0, n), perm


def runoff_of(n, seed, nmonths=4):
    rng = np.random.default_rng(seed)
    q = rng.gamma(2.0, 30.0, (n, nmonths))
    q[:, 2] *= 0.02                                         # a dry month
    return q


def route_both(csr, L, v, area, q, ndays=FOUR, spin=0):
    """The call by the library's default form on the prepared plan, the oracle's result, the plan."""
    from oracle import mrtm as o_mrtm
    from xanthos_amd import _hip
    from xanthos_amd.routing import mrtm
    um = mrtm.UpstreamMatrix(*csr)
    ref = o_mrtm.route_series(um.tocsr(), L, v, area, q, ndays, spin)
    got = mrtm.route_series(um, L, v, area, q, ndays, spin)
    return got, ref, um.plan(_hip.get_context())


def assert_within_bar(got, ref):
    for name, x, r, atol in zip(('ChStorage', 'Avg_ChFlow', 'F_end'), got, ref, BAR):
        assert np.array_equal(np.isnan(x), np.isnan(r)), name + ': NaN masks differ'
        m = ~np.isnan(r)
        err = np.abs(x[m] - r[m])
        bound = 1e-9 * np.abs(r[m]) + atol
        print('%s: largest |x - ref| %.3e, largest excess over the bar %.3e' % (name, err.max() if err.size else 0.0,
                                                                               (err - bound).max() if err.size else 0.0))
        assert (err <= bound).all(), (name, float((err - bound).max()))


def test_world_without_a_cell_that_may_fire_runs_linear_units_only():
    ds, L, v, area = quiet_world()
    got, ref, plan = route_both(csr_of(ds), L, v, area, runoff_of(len(ds), 11))
    info, ri = plan.info(), plan.rsum_info()
    print(info, ri)
    assert info['last_tree_kernel'] == 4 and info['reroutes'] == 0, info
    assert ri['pair_cells'] == 0 and ri['pair_units'] == 0, ri               # a single-sum plan without pair units ...
    assert ri['units'] >= 3 and ri['linear_units'] == ri['units'], ri        # ... all of whose units ran the linear step
    assert ri['guard_trips'] == 0 and ri['fold_disabled'] == 0, ri
    assert_within_bar(got, ref)


def test_corner_world_mixes_the_forms():
    """tests/corner_world.py: cells that can fire, halos, pair units, and tributaries that cannot fire; the guard stays quiet."""
    import corner_world as cw
    idx, csr, L, v, area = cw.make(seed=3)
    q = cw.runoff(len(L), nmonths=4, seed=3)
    fired, neg_s, _ = cw.instrumented(csr, L, v, area, q, FOUR)
    assert fired.sum() > 0 and (neg_s > 0).sum() >= 1                          # the corner does occur in these four months
    got, ref, plan = route_both(csr, L, v, area, q)
    info, ri = plan.info(), plan.rsum_info()
    print(info, ri)
    assert info['last_tree_kernel'] == 4 and info['reroutes'] == 0, info
    assert ri['pair_cells'] > 0 and ri['pair_units'] >= 1, ri
    assert 1 <= ri['linear_units'] <= ri['units'] - ri['pair_units'], ri      # (the host planner on this world: 2 pair units, 3 linear)
    assert ri['guard_trips'] == 0 and ri['fold_disabled'] == 0, ri
    assert_within_bar(got, ref)


def test_two_import_rounds_and_both_outlet_forms():
    ds, L, v, area, _ = comb_world()
    got, ref, plan = route_both(csr_of(ds), L, v, area, runoff_of(len(ds), 12))
    info, ri = plan.info(), plan.rsum_info()
    print(info, ri)
    assert info['last_tree_kernel'] == 4 and info['reroutes'] == 0, info
    assert info['flow_max_imports'] >= 9, info                                 # NG = 2 runs; its unit has no outlet (NXR = 0) ...
    assert info['flow_edges'] >= 9 and ri['linear_units'] == ri['units'], (info, ri)      # ... its producers have one (NXR = 1)
    assert ri['guard_trips'] == 0 and ri['fold_disabled'] == 0, ri
    assert_within_bar(got, ref)


def test_nan_runoff_upstream_of_linear_units():
    """A cell whose runoff is NaN from the second month on, at the head of a tributary of the comb: everything downstream of it
    turns NaN as the oracle's does, month by month, across units (the stream carries the NaN) -- and the guard ignores it."""
    ds, L, v, area, perm = comb_world()
    q = runoff_of(len(ds), 13)
    head = int(perm[13 + 63])                                 # the last cell of the first tributary: far upstream
    q[head, 1:] = np.nan
    got, ref, plan = route_both(csr_of(ds), L, v, area, q)
    ri = plan.rsum_info()
    print(ri)
    assert np.isnan(ref[0]).any() and not np.isnan(ref[0]).all()              # NaN downstream of the cell, numbers elsewhere
    assert np.isnan(ref[0][int(perm[0])]).any()                               # ... down to the outlet of the stem
    assert ri['linear_units'] == ri['units'] and ri['guard_trips'] == 0 and ri['fold_disabled'] == 0, ri
    assert_within_bar(got, ref)


def test_negative_storage_trips_the_guard_and_the_call_is_rerouted():
    """Runoff negative enough to take a storage below zero in a unit that runs the linear step: the reference fires there
    (mrtm.py:54), the linear step may not be used -- the unit gives up, the call is routed again on the plan of pairs, and the
    result is within the bar all the same.  (Negative runoff also trips the plan's older guard on the lateral inflow, a month
    ahead of the storage: with non-negative inputs the older guards already imply S1 >= 0, so no input reaches the storage
    guard alone; `guard_trips` counts the call, whichever guard of the unit spoke first.)"""
    import corner_world as cw
    ds, L, v, area = quiet_world()
    n = len(ds)
    q = runoff_of(n, 14)
    cell = int(np.flatnonzero(ds >= 0)[5])
    q[cell, 2] = -40.0                                        # mm in the dry month: more than the cell holds and receives
    fired, neg_s, _ = cw.instrumented(csr_of(ds), L, v, area, q, FOUR)
    assert fired[cell] > 0                                    # the oracle's trial storage does go negative in that cell
    got, ref, plan = route_both(csr_of(ds), L, v, area, q)
    info, ri = plan.info(), plan.rsum_info()
    print(info, ri)
    assert info['last_tree_kernel'] == 4, info
    assert ri['guard_trips'] >= 1 and ri['fold_disabled'] == 1 and ri['pair_cells'] == -1 and ri['linear_units'] == 0, ri
    assert_within_bar(got, ref)
