"""GPU tests of the csv formatter (csrc/xh_csv.hip on csrc/xh_dtoa.h) and of the writers on it: the text formatted in HBM
against CPython's repr and the host loop of OutWriter.write_data, restated in tests/csv_np.py -- bytes and row offsets."""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_np  # noqa: E402
import writer_np as W  # noqa: E402

from oracle import writer as o_writer  # noqa: E402
from xanthos_amd import _hip  # noqa: E402
from xanthos_amd.data_writer.out_writer import OutWriter  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return _hip.get_context(0)


def check_format(ctx, table, first_id, tag=''):
    d = ctx.upload(table)
    try:
        text, offsets = ctx.csv_format(d, first_id=first_id)
    finally:
        d.free()
    want = csv_np.body(table, first_id)
    assert np.array_equal(offsets, csv_np.row_offsets(table, first_id)), tag
    if text != want:
        for k, (a, b) in enumerate(zip(text.split(b'\n'), want.split(b'\n'))):
            assert a == b, '{}: line {}: {!r} instead of {!r}'.format(tag, k, a[:200], b[:200])
    assert text == want, tag


def sample(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == 'hand':
        return np.resize(csv_np.hand_list(), n)
    if kind == 'bits':
        return csv_np.random_bits(n, seed)
    if kind == 'gamma':                                   # like runoff and flows: positive, a few zeros and NaN
        v = rng.gamma(0.7, 40.0, n)
        v[rng.random(n) < 0.02] = 0.0
        v[rng.random(n) < 0.01] = np.nan
        return v
    return rng.normal(0.0, 1e3, n)


@pytest.mark.parametrize('first_id', [0, 1, 99999])
@pytest.mark.parametrize('nrows', [1, 3, 257])
@pytest.mark.parametrize('ncols', [1, 2, 63, 64, 65, 600])
def test_format_shapes(ctx, ncols, nrows, first_id):
    """Every shape at which the strip loop, the wave scan and the aligned stores' head and tail change, with ids whose
    width changes inside the array (99,999 -> 100,000), on values of every kind."""
    kinds = ('hand', 'bits', 'gamma', 'normal')
    n = nrows * ncols
    vals = np.concatenate([sample(k, n // 4 + 1, 1000 * ncols + nrows + i) for i, k in enumerate(kinds)])
    np.random.default_rng(ncols + nrows).shuffle(vals)
    check_format(ctx, vals[:n].reshape(nrows, ncols), first_id, (ncols, nrows, first_id))


def test_format_hand_list(ctx):
    """The whole hand list: specials, subnormals, the layout switches, powers of two and ten, integers to 2^53."""
    check_format(ctx, csv_np.as_table(csv_np.hand_list(), 65), 1, 'hand list')


def test_format_random_bit_patterns(ctx):
    """500,000 random 64-bit patterns."""
    check_format(ctx, csv_np.random_bits(500000, 7).reshape(2000, 250), 1, 'random bits')


@pytest.mark.parametrize('kind', ['gamma', 'normal'])
def test_format_values_like_outputs(ctx, kind):
    check_format(ctx, sample(kind, 400 * 600, 5).reshape(400, 600), 1, kind)


def test_format_all_nan_and_longest_rows(ctx):
    """Lines of commas only, and rows of 600 fields of 24 characters, the longest there is (beyond one LDS image)."""
    check_format(ctx, np.full((5, 600), np.nan), 8, 'NaN')
    check_format(ctx, np.full((3, 1), np.nan), 0, 'NaN, one column')
    long = -np.abs(csv_np.random_bits(20000, 3))
    long = long[[len(csv_np.field(v)) == 24 for v in long]][:4 * 600].reshape(4, 600)
    assert long.shape == (4, 600)
    check_format(ctx, long, 99998, '24 characters')


def test_format_refuses_a_short_buffer(ctx):
    d = ctx.upload(np.ones((4, 4)))
    with pytest.raises(_hip.HipError, match='error 3'):
        ctx.csv_format(d, cap=16)
    assert ctx.csv_format(d)[0] == csv_np.body(np.ones((4, 4)), 1)
    d.free()


def test_write_in_chunks_behind_a_header(ctx, tmp_path):
    """257 x 65 in five and more chunks equals the one-chunk file; the text starts at ``offset`` behind a header, the file
    is not truncated and bytes_written is its growth."""
    table = sample('gamma', 257 * 65, 77).reshape(257, 65)
    table[5] = sample('bits', 65, 78)
    want = csv_np.body(table, 1)
    d = ctx.upload(table)
    one, many = str(tmp_path / 'one.csv'), str(tmp_path / 'many.csv')
    assert ctx.csv_write(one, d) == len(want)               # the file is created
    assert open(one, 'rb').read() == want
    header = b'id,' + b','.join(b'%d' % k for k in range(65)) + b'\n'
    tail = b'#' * 1000
    with open(many, 'wb') as fh:
        fh.write(header + b'?' * len(want) + tail)
    chunk = len(want) // 6
    assert len(want) / chunk >= 5
    assert ctx.csv_write(many, d, first_id=1, offset=len(header), chunk_bytes=chunk) == len(want)
    assert open(many, 'rb').read() == header + want + tail
    tiny = str(tmp_path / 'tiny.csv')                        # a chunk smaller than a line: a line at a time
    assert ctx.csv_write(tiny, d, chunk_bytes=10) == len(want)
    assert open(tiny, 'rb').read() == want
    d.free()


def test_write_many_equals_single_writes(ctx, tmp_path):
    tables = [sample('gamma', 100 * 36, 1).reshape(100, 36), sample('bits', 7 * 600, 2).reshape(7, 600),
              sample('normal', 1000, 3).reshape(1000, 1)]
    firsts = [1, 0, 99990]
    devs = [ctx.upload(t) for t in tables]
    paths = [str(tmp_path / 'f{}.csv'.format(k)) for k in range(3)]
    written = ctx.csv_write_many([(p, d, f, 0) for p, d, f in zip(paths, devs, firsts)], chunk_bytes=4096)
    for k, (p, d, f) in enumerate(zip(paths, devs, firsts)):
        single = str(tmp_path / 's{}.csv'.format(k))
        assert ctx.csv_write(single, d, first_id=f) == written[k]
        got = open(p, 'rb').read()
        assert got == open(single, 'rb').read() == csv_np.body(tables[k], f), k
        d.free()


def test_unwritable_path_leaves_the_context_usable(ctx, tmp_path):
    d = ctx.upload(np.ones((3, 3)))
    with pytest.raises(_hip.HipError, match='error 1.*No such file or directory'):
        ctx.csv_write(str(tmp_path / 'no' / 'such' / 'folder' / 'a.csv'), d)
    assert ctx.csv_format(d)[0] == csv_np.body(np.ones((3, 3)), 1)
    d.free()


def settings(folder, years, in_year, unit):
    return NS(output_vars=['q', 'avgchflow'], ProjectName='p', OutputFolder=str(folder), OutputFormat=1,
              OutputUnit=unit, OutputInYear=in_year, StartYear=2001, EndYear=2000 + years, device=0)


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('unit', [0, 1], ids=['mm', 'km3'])
@pytest.mark.parametrize('in_year', [0, 1], ids=['month', 'year'])
def test_out_writer_formats_in_hbm(ctx, tmp_path, golden, monkeypatch, in_year, unit, device):
    """OutWriter.write() on the hostile world of writer_hostile.npz: no array crosses PCIe as doubles (DeviceArray.download
    raises while write() runs), and every csv file is what the host loop makes of the same values."""
    h = golden('writer_hostile')
    q, area = h['q'], h['area']
    ac = W.hostile(np.random.default_rng(3), *q.shape)
    years = q.shape[1] // 12
    src = {'q': ctx.upload(q), 'avgchflow': ctx.upload(ac)} if device else {'q': q, 'avgchflow': ac}
    w = OutWriter(settings(tmp_path, years, in_year, unit), area, src)

    def refuse(self, out=None):
        raise AssertionError('write() downloaded an array')
    with monkeypatch.context() as m:
        m.setattr(_hip.DeviceArray, 'download', refuse)
        w.write()
    want_q = o_writer.agg_to_year(q, 'sum') if in_year else q
    if unit:
        want_q = o_writer.mm_to_km3(want_q, area)
    want = {'q': want_q, 'avgchflow': o_writer.agg_to_year(ac, 'mean') if in_year else ac}
    steps = [str(2001 + y) for y in range(years)] if in_year else \
        ['{}{:02}'.format(2001 + y, m) for y in range(years) for m in range(1, 13)]
    unit_str = '{}per{}'.format(('mm', 'km3')[unit], ('month', 'year')[in_year])
    for var in ('q', 'avgchflow'):
        path = os.path.join(str(tmp_path), '{}_{}_p.csv'.format(var, 'm3persec' if var == 'avgchflow' else unit_str))
        assert open(path, 'rb').read() == csv_np.file_bytes(want[var], steps, 1), var
        got = w.get(var)                                   # host arrays on demand
        assert isinstance(got, np.ndarray) and np.array_equal(got, want[var], equal_nan=True), var
    if device:
        for a in src.values():
            a.free()


def test_ensemble_csv_files_equal_the_host_loop(tmp_path):
    """run_ensemble with csv member outputs and the mean: every member and statistics file is the host loop's text of
    the values the same ensemble writes as npy."""
    from xanthos_amd import run_ensemble, synth
    years, trees = 3, {}
    for fmt in (1, 4):
        root = str(tmp_path / 'fmt{}'.format(fmt))
        w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=33)
        forcings = [synth.make_forcing(w, 12 * years, seed=100 + 7 * k) for k in range(2)]
        ini, _ = synth.write_ensemble_example(root, w, forcings, 1971, 1970 + years, runoff_spinup=25, routing_spinup=6,
                                              statistics=('mean',), output_format=fmt)
        res = run_ensemble(ini)
        trees[fmt] = os.path.join(root, 'output', 'pm_abcd_mrtm_synth')
        assert len(res.names) == 2
    steps = ['{}{:02}'.format(1971 + y, m) for y in range(years) for m in range(1, 13)]
    seen = 0
    for base, _, names in os.walk(trees[4]):
        for n in names:
            if n.endswith('.npy'):
                values = np.load(os.path.join(base, n))
                twin = os.path.join(trees[1], os.path.relpath(base, trees[4]), n[:-4] + '.csv')
                assert open(twin, 'rb').read() == csv_np.file_bytes(values, steps, 1), twin
                seen += 1
    assert seen >= 3 * 2                                    # members and ensemble/, q and avgchflow at the least
