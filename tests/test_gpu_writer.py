"""GPU tests of the output writer (data_writer/out_writer.py on csrc/xh_agg.hip and xh_diag_group_sum) against pandas'
summation order, bit for bit: the oracle (oracle/writer.py, itself held to the reference and to pandas by
test_oracle_golden.py) and the reference's own values in tests/golden/writer_hostile.npz.  The inputs are hostile
(tests/writer_np.py): years and basins whose sums depend on the order, NaN, +/-inf, -0.0 and subnormals.  The last test
pins the plain order that the time-series tables and accessible water keep."""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import writer_np as W  # noqa: E402

from oracle import writer as o_writer  # noqa: E402
from xanthos_amd import _hip  # noqa: E402
from xanthos_amd.data_writer.out_writer import OutWriter  # noqa: E402

pytestmark = pytest.mark.gpu

FULL_CELLS = 67420


def same(x, ref, tag=''):
    """Bit for bit, NaN where NaN, and the sign of zeros too."""
    x, ref = np.asarray(x), np.asarray(ref)
    assert x.shape == ref.shape, (tag, x.shape, ref.shape)
    bad = ~((x == ref) | (np.isnan(x) & np.isnan(ref)))
    assert not bad.any(), '{}: {} of {} values differ, first at {}: {!r} vs {!r}'.format(
        tag, int(bad.sum()), bad.size, np.argwhere(bad)[0], x[bad][0], ref[bad][0])
    m = ~np.isnan(ref)
    assert np.array_equal(np.signbit(x[m]), np.signbit(ref[m])), tag + ': the sign of a zero differs'


def settings(tmp_path, years=1, in_year=1, unit=0, fmt=4, start=2001):
    return NS(output_vars=['q', 'avgchflow'], ProjectName='p', OutputFolder=str(tmp_path), OutputFormat=fmt,
              OutputUnit=unit, OutputInYear=in_year, StartYear=start, EndYear=start + years - 1, device=0)


def writer(tmp_path, ncell, **kw):
    return OutWriter(settings(tmp_path, **kw), np.ones(ncell), {})


@pytest.mark.parametrize('nm', [12, 24, 600, 1200])
@pytest.mark.parametrize('ncell', [1, 255, 256, 257, 5000])
def test_agg_to_year_bit_exact(tmp_path, ncell, nm):
    """Yearly sums and means, with and without the km3 scale, equal pandas' compensated order for every value."""
    rng = np.random.default_rng(ncell * 7919 + nm)
    q = W.hostile(rng, ncell, nm)
    area = rng.uniform(800, 3100, ncell)
    w = writer(tmp_path, ncell)
    ysum, ymean = o_writer.agg_to_year(q, 'sum'), o_writer.agg_to_year(q, 'mean')
    got = w.agg_to_year(q, 'sum')
    same(got, ysum, 'sum')
    assert got[0, 0] == 10.0                                       # [1e16, 1, 1, -1e16, 1 x 8]; a plain sum gives 8.0
    same(w.agg_to_year(q, 'mean'), ymean, 'mean')
    same(w.agg_to_year(q, 'sum', scale=area / 1e6), o_writer.mm_to_km3(ysum, area), 'sum km3')
    same(w.agg_to_year(q, 'mean', scale=area / 1e6), o_writer.mm_to_km3(ymean, area), 'mean scaled')


def test_hostile_fixture_on_device(tmp_path, golden):
    """The reference's OutWriter values of writer_hostile.npz, every one."""
    h = golden('writer_hostile')
    q, area, ids, n = h['q'], h['area'], h['ids'], int(h['n_names'])
    w = writer(tmp_path, q.shape[0])
    ysum = w.agg_to_year(q, 'sum')
    same(ysum, h['ysum'], 'ysum')
    assert ysum[0, 0] == 10.0
    same(w.agg_to_year(q, 'mean'), h['ymean'], 'ymean')
    same(w._agg(q, 1, 0, area / 1e6), h['km3'], 'km3')
    same(w.agg_to_year(q, 'sum', scale=area / 1e6), h['ysum_km3'], 'ysum_km3')
    same(w.agg_spatial(q, ids, n, first_id=1), h['spatial1'], 'spatial from 1')
    same(w.agg_spatial(q, ids, n, first_id=0), h['spatial0'], 'spatial from 0')
    same(w.agg_spatial(h['ysum_km3'], ids, n, first_id=1), h['spatial_year'], 'spatial of the year sums')
    d_q = _hip.get_context(0).upload(q)                             # a device-resident input
    same(w.agg_to_year(d_q, 'sum'), h['ysum'], 'ysum from HBM')
    same(w.agg_spatial(d_q, ids, n, first_id=0), h['spatial0'], 'spatial from HBM')
    d_q.free()


def test_agg_spatial_cases(tmp_path):
    """Single-cell groups, a group of half the full grid, names without cells, dropped ids (0, -9999, beyond the names),
    names from 0 and from 1, +inf with -inf in one group (NaN) and a lone inf (inf)."""
    rng = np.random.default_rng(77)
    w = writer(tmp_path, 1)
    # single-cell groups: a group of one value v sums to 0.0 + v
    q = W.hostile(rng, 300, 24)
    ids = np.arange(1, 301)
    same(w.agg_spatial(q, ids, 300), o_writer.agg_spatial(q, ids, 300), 'single cells')
    same(w.agg_spatial(q, ids, 300), np.where(np.isnan(q), 0.0, q + 0.0), 'single cells, restated')
    # one group holds half of a full-size grid; the others are small, one name has no cells, some ids are dropped
    q = W.hostile(rng, FULL_CELLS, 24)
    ids = rng.integers(2, 60, FULL_CELLS)
    ids[rng.permutation(FULL_CELLS)[:FULL_CELLS // 2]] = 1
    ids[ids == 7] = 8
    ids[rng.random(FULL_CELLS) < 0.01] = 0
    ids[rng.random(FULL_CELLS) < 0.01] = -9999
    for first, n in ((1, 50), (0, 50), (1, 70)):
        ref = o_writer.agg_spatial(q, ids, n, first_id=first)
        got = w.agg_spatial(q, ids, n, first_id=first)
        same(got, ref, 'half grid, first_id {}, {} names'.format(first, n))
        assert np.isnan(got[7 - first]).all()                       # name 7: no cells
        if n == 70:
            assert np.isnan(got[60 - first:]).all()                 # names beyond the ids
    # infinities: +inf with -inf in one group gives NaN, a lone inf stays inf, a lone -inf stays -inf
    q = np.ones((6, 3))
    q[0, 0], q[1, 0], q[2, 1], q[4, 2], q[5, 2] = np.inf, -np.inf, np.inf, -np.inf, np.nan
    ids = np.array([1, 1, 1, 2, 2, 2])
    got = w.agg_spatial(q, ids, 3)
    same(got, o_writer.agg_spatial(q, ids, 3), 'infinities')
    assert np.isnan(got[0, 0]) and got[0, 1] == np.inf and got[1, 2] == -np.inf and np.isnan(got[2]).all()


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('fmt', [1, 4], ids=['csv', 'npy'])
@pytest.mark.parametrize('unit', [0, 1], ids=['mm', 'km3'])
@pytest.mark.parametrize('in_year', [0, 1], ids=['month', 'year'])
def test_write_files(tmp_path, in_year, unit, fmt, device):
    """write(): runoff summed per year (and converted to km3), channel flow averaged per year and never converted; the
    files (npy, or csv parsed back: repr round-trips a double exactly) hold the oracle's values."""
    rng = np.random.default_rng(11 + 2 * in_year + 4 * unit + 8 * fmt + int(device))
    ncell, years = 333, 3
    q, ac = W.hostile(rng, ncell, 12 * years), W.hostile(rng, ncell, 12 * years)
    area = rng.uniform(800, 3100, ncell)
    ctx = _hip.get_context(0)
    src = {'q': ctx.upload(q), 'avgchflow': ctx.upload(ac)} if device else {'q': q, 'avgchflow': ac}
    w = OutWriter(settings(tmp_path, years=years, in_year=in_year, unit=unit, fmt=fmt), area, src)
    w.write()
    want_q = o_writer.agg_to_year(q, 'sum') if in_year else q
    if unit:
        want_q = o_writer.mm_to_km3(want_q, area)
    want = {'q': want_q, 'avgchflow': o_writer.agg_to_year(ac, 'mean') if in_year else ac}
    unit_str = '{}per{}'.format(('mm', 'km3')[unit], ('month', 'year')[in_year])
    steps = [str(2001 + y) for y in range(years)] if in_year else \
        ['{}{:02}'.format(2001 + y, m) for y in range(years) for m in range(1, 13)]
    for var in ('q', 'avgchflow'):
        same(w.get(var), want[var], var + ' get')
        path = os.path.join(str(tmp_path), '{}_{}_p'.format(var, 'm3persec' if var == 'avgchflow' else unit_str))
        if fmt == 4:
            same(np.load(path + '.npy'), want[var], var + ' npy')
        else:
            lines = open(path + '.csv').read().splitlines()
            assert lines[0] == 'id,' + ','.join(steps)
            assert len(lines) == ncell + 1
            rows = [ln.split(',') for ln in lines[1:]]
            assert [int(r[0]) for r in rows] == list(range(1, ncell + 1))
            vals = np.array([[float(v) if v != '' else np.nan for v in r[1:]] for r in rows])
            same(vals, want[var], var + ' csv')
    if device:
        for a in src.values():
            a.free()


def test_full_size_years(tmp_path):
    """67,420 cells x 600 months: every yearly sum and mean bit for bit."""
    rng = np.random.default_rng(67420)
    q = W.hostile(rng, FULL_CELLS, 600)
    w = writer(tmp_path, FULL_CELLS)
    d_q = _hip.get_context(0).upload(q)
    same(w.agg_to_year(d_q, 'sum'), o_writer.agg_to_year(q, 'sum'), 'full-size sum')
    same(w.agg_to_year(d_q, 'mean'), o_writer.agg_to_year(q, 'mean'), 'full-size mean')
    d_q.free()


def test_plain_orders_stay_plain(tmp_path):
    """The group [1e16, 1, 1] tells the orders apart: the time-series tables and accessible water add plainly (their
    references are plain loops) and give 1e16; the writer adds in pandas' compensated order and gives 1e16 + 2."""
    from xanthos_amd.accessible import accessible
    from xanthos_amd.diagnostics import time_series
    ctx = _hip.get_context(0)
    cells = np.array([[1e16], [1.0], [1.0]])
    ids = np.array([1, 1, 1])
    assert time_series.Aggregation_Map(ids, cells, ctx)[0, 0] == 1e16
    monthly = np.zeros((3, 12))
    monthly[:, 0] = cells[:, 0]
    assert accessible.basin_year_totals(ctx, monthly, np.full(3, 1e6), ids)[0, 0] == 1e16
    got = writer(tmp_path, 3).agg_spatial(cells, ids, 1)[0, 0]
    assert got == 1.0000000000000002e16 == o_writer.agg_spatial(cells, ids, 1)[0, 0]
