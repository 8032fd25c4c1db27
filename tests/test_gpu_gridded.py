"""GPU (-m gpu): gridded CF NetCDF maps written from HBM ([Project] GriddedOutput = 1).

xh_grid_pack_f32_be against the numpy restatement of tests/grid_np.py byte for byte; OutWriter with a grid map next to
its per-cell files, from host arrays and from DeviceArrays; run_model() and run_ensemble() with the key set against
their own npy outputs.  tests/test_gridded_host.py pins the map, the header and the key without a GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_np  # noqa: E402

pytestmark = pytest.mark.gpu

SPECIAL = (np.nan, 0.0, 1e-40, 1e-45, 7e-46, 1e39, 3.4028235677973366e38, 3.4028234e38, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24)
NC, CSV, NPY = 0, 1, 4
EXT = {NC: '.nc', CSV: '.csv', NPY: '.npy'}
VARS = ('q', 'avgchflow', 'soilmoisture')
CASES = {'m0': (0, 0), 'y1': (1, 1)}                 # (OutputInYear, OutputUnit)
PROJECT = 'pm_abcd_mrtm_synth'


def read(path):
    with open(path, 'rb') as fh:
        return fh.read()


def coords_of(nrow, ncol, ncell, seed, columns=None):
    """A coordinates table of ``ncell`` cells on distinct slots, slot 0 and the last slot among them, in the column-major
    order of the reference's table (so cell order is not slot order); ``columns``: the grid columns that may hold cells."""
    rng = np.random.default_rng(seed)
    cand = np.arange(nrow * ncol)
    if columns is not None:
        cand = cand[np.isin(cand % ncol, columns)]
    inner = cand[(cand != 0) & (cand != nrow * ncol - 1)]
    ends = np.unique([0, nrow * ncol - 1])[:ncell]
    slots = np.concatenate([ends, rng.choice(inner, ncell - len(ends), replace=False)])
    rows, cols = slots // ncol, slots % ncol
    perm = np.lexsort((rows, cols))
    rows, cols = rows[perm], cols[perm]
    lat, lon = -90 + (rows + .5) * 180 / nrow, -180 + (cols + .5) * 360 / ncol
    return np.stack([np.arange(1, ncell + 1), lon, lat, cols + 1, rows + 1], axis=1).astype(float)


def values(ncell, ncols, seed):
    """The special values and their negatives lead (a different one first at every shape), random values of every binary32
    exponent and beyond on both sides follow; from the third row on one NaN lies inside a land cell."""
    rng = np.random.default_rng(seed)
    n = ncell * ncols
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-50, 42, n)
    special = np.array([v for s in SPECIAL for v in (s, -s)])
    k = min(n, special.size)
    a[:k] = special[(seed % special.size + np.arange(k)) % special.size]
    a = a.reshape(ncell, ncols)
    if ncell > 2:
        a[ncell // 2, ncols // 2] = np.nan
    return a


# ---- the kernel alone
SHAPES = [(1, 1, 1, 1), (5, 7, 17, 3), (9, 15, 40, 65), (20, 33, 200, 130), (3, 300, 64, 24)]


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(str(n) for n in s) for s in SHAPES])
def test_grid_pack_equals_numpy(shape):
    """(1, 1, 1, 1): one value; (5, 7, 17, 3): 35 slots, below one tile of 64, rows of three doubles (8-byte aligned only);
    (9, 15, 40, 65): two tiles of slots and seven, one time step past 64; (20, 33, 200, 130): ten tiles and 20, two tiles
    of time and two; (3, 300, 64, 24): the cells in the first and last 32 columns, whole tiles of ocean between them."""
    from xanthos_amd import _hip
    nrow, ncol, ncell, ncols = shape
    ctx = _hip.get_context(0)
    columns = np.r_[0:32, ncol - 32:ncol] if ncol == 300 else None
    coords = coords_of(nrow, ncol, ncell, seed=ncell, columns=columns)
    table = grid_np.cell_of_slot(coords, nrow, ncol)
    nslots = nrow * ncol
    assert table[0] >= 0 and table[-1] >= 0 and (table >= 0).sum() == ncell and table.max() == ncell - 1
    if ncell > 2:
        assert not (np.diff(grid_np.slot_of_cell(coords, ncol)) > 0).all()
    if columns is not None:
        assert (table.reshape(-1)[64:128] < 0).all()              # a whole tile without a cell
    a = values(ncell, ncols, seed=ncell + 3)              # (1 x 1: the one value is 1e-40, a binary32 subnormal)
    ref = grid_np.grid_body(a, table).tobytes()
    src, tab = ctx.upload(a), ctx.upload(table, dtype=np.int32)
    dst = ctx.empty((ncols * nslots + 4,), dtype=np.uint32)       # (and four words behind the body: they stay as they are)
    try:
        dst.zero()
        ctx.grid_pack_f32_be(src, tab, nslots, grid_np.FILL_BITS, dst)
        got = dst.download().tobytes()
        assert got[:len(ref)] == ref and got[len(ref):] == b'\x00' * 16
        with pytest.raises(_hip.HipError, match='aligned'):
            ctx.grid_pack_f32_be(src, tab, nslots, grid_np.FILL_BITS, dst.ptr + 4)
        with pytest.raises(_hip.HipError, match='bad argument'):
            ctx.grid_pack_f32_be(src, tab, 0, grid_np.FILL_BITS, dst)
    finally:
        for b in (src, tab, dst):
            b.free()


# ---- the writer
@pytest.fixture(scope='module')
def small():
    """900 cells on 36 x 72, 24 months of the three variables (a NaN in each) and the cells' areas."""
    from xanthos_amd import synth
    from xanthos_amd.data_writer.gridded import GridMap
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=21)
    rng = np.random.default_rng(4)
    arrays = {v: rng.random((900, 24)) * 300 for v in VARS}
    for k, v in enumerate(VARS):
        arrays[v][10 + k, 3] = np.nan
    return SimpleNamespace(world=w, grid=GridMap(w.coords, 36, 72), arrays=arrays, area=w.area)


def settings(folder, fmt, case):
    in_year, unit = CASES[case]
    return SimpleNamespace(output_vars=list(VARS), ProjectName='maps', OutputFolder=str(folder), OutputFormat=fmt,
                           OutputUnit=unit, OutputInYear=in_year, StartYear=1899, EndYear=1900, device=0)


@pytest.mark.parametrize('device', [False, True], ids=['host', 'hbm'])
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('fmt', [NC, CSV, NPY], ids=['nc', 'csv', 'npy'])
def test_writer_with_a_grid(small, tmp_path, fmt, case, device):
    from xanthos_amd import _hip
    from xanthos_amd.data_writer import gridded
    from xanthos_amd.data_writer.out_writer import OutWriter
    ctx = _hip.get_context(0)
    folders = {with_grid: tmp_path / ('grid' if with_grid else 'plain') for with_grid in (False, True)}
    in_year = CASES[case][0]
    for with_grid, folder in folders.items():
        inputs = {v: (ctx.upload(small.arrays[v]) if device else small.arrays[v].copy()) for v in VARS}
        w = OutWriter(settings(folder, fmt, case), small.area, inputs, grid=small.grid if with_grid else None)
        w.write()
        assert w._grids_from_device is None
        if with_grid:
            days, units = gridded.time_axis(1899, 2 if in_year else 24, in_year)
            for var in VARS:
                stem = '{}_{}_maps'.format(var, w.unit_of(var))
                header = gridded.grid_nc_header(var, w.unit_of(var), days, units, small.grid, title='maps')
                assert read(str(folder / (stem + '_grid.nc'))) == header + grid_np.grid_body(w.get(var), small.grid.cell_of_slot).tobytes(), var
        for a in inputs.values():
            if device:
                a.free()
    plain, grid = sorted(os.listdir(str(folders[False]))), sorted(os.listdir(str(folders[True])))
    assert len(plain) == 3 and all(n.endswith(EXT[fmt]) for n in plain)
    assert grid == sorted(plain + [n[:-len(EXT[fmt])] + '_grid.nc' for n in plain])
    for n in plain:
        assert read(str(folders[False] / n)) == read(str(folders[True] / n)), n


def test_writer_outside_write_and_tables_with_names(small, tmp_path):
    """The statistics' route (write_data outside write()) writes the map at once; a table with names, an array of another
    height and write_files = False write none."""
    from xanthos_amd.data_writer.out_writer import OutWriter
    w = OutWriter(settings(tmp_path, CSV, 'm0'), small.area, {}, grid=small.grid)
    dev = w.ctx.upload(small.arrays['q'])
    w.write_data(str(tmp_path / 'q_stat'), 'q', dev, w.time_steps)
    dev.free()
    assert read(str(tmp_path / 'q_stat_grid.nc')).endswith(grid_np.grid_body(small.arrays['q'], small.grid.cell_of_slot).tobytes())
    w.write_data(str(tmp_path / 'basins'), 'Basin_runoff', np.ones((7, 24)), w.time_steps, names=['b'] * 7)
    w.write_data(str(tmp_path / 'short'), 'q', np.ones((7, 24)), w.time_steps)
    w.write_data(str(tmp_path / 'named'), 'q', small.arrays['q'], w.time_steps, names=['c'] * 900)
    w.write_files = False
    w.write_data(str(tmp_path / 'off'), 'q', small.arrays['q'], w.time_steps)
    assert sorted(n for n in os.listdir(str(tmp_path)) if n.endswith('_grid.nc')) == ['q_stat_grid.nc']


# ---- whole runs
@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """The world, two forcing sets and the single run of each with GriddedOutput = 1 (npy): {k: output folder}."""
    from xanthos_amd import run_model, synth
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=33)
    forcings = [synth.make_forcing(w, 36, seed=100 + 7 * k) for k in range(2)]
    out = {}
    for k, f in enumerate(forcings):
        root = str(tmp_path_factory.mktemp('single{}'.format(k)))
        run_model(synth.write_example(root, w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, output_format=NPY,
                                      output_vars=VARS, gridded=True))
        out[k] = os.path.join(root, 'output', PROJECT)
    return SimpleNamespace(world=w, forcings=forcings, out=out)


def files_of(folder):
    return {n: read(os.path.join(folder, n)) for n in sorted(os.listdir(folder))
            if n != 'logfile.log' and os.path.isfile(os.path.join(folder, n))}


def test_run_model_writes_the_maps(runs, tmp_path):
    from xanthos_amd import run_model, synth
    w, out = runs.world, runs.out[0]
    slots = grid_np.slot_of_cell(w.coords, 72)
    ocean = grid_np.cell_of_slot(w.coords, 36, 72) < 0
    names = sorted(os.listdir(out))
    maps = [n for n in names if n.endswith('_grid.nc')]
    assert maps == sorted('{}_{}_{}_grid.nc'.format(v, 'm3persec' if v == 'avgchflow' else 'mmpermonth', PROJECT) for v in VARS)
    for n in maps:
        var = n.split('_')[0]
        dims, glob, variables = grid_np.contents(os.path.join(out, n))
        assert dims == [('time', 36), ('lat', 36), ('lon', 72)] and glob['title'] == PROJECT.encode()
        assert np.frombuffer(variables['time'][3], '>i4').tolist() == grid_np.time_days(1971, 36, 0)
        cube = np.frombuffer(variables[var][3], '>f4').reshape(36, -1)
        per_cell = np.load(os.path.join(out, n[:-len('_grid.nc')] + '.npy'))
        narrowed = per_cell.astype('>f4')
        narrowed[np.isnan(per_cell)] = grid_np.FILL           # (a NaN of the model's own is a missing value of the map)
        assert per_cell.shape == (900, 36) and cube[:, slots].T.tobytes() == narrowed.tobytes(), n
        assert (cube[:, ocean].view('>u4') == grid_np.FILL_BITS).all() and ocean.sum() == 36 * 72 - 900
    # the same ini with the key at 0: the same folder without the maps
    root = str(tmp_path / 'off')
    ini = synth.write_example(root, w, runs.forcings[0], 1971, 1973, runoff_spinup=25, routing_spinup=6, output_format=NPY,
                              output_vars=VARS, gridded=True)
    text = open(ini).read()
    assert 'GriddedOutput = 1' in text
    with open(ini, 'w') as fh:
        fh.write(text.replace('GriddedOutput = 1', 'GriddedOutput = 0'))
    run_model(ini)
    off = files_of(os.path.join(root, 'output', PROJECT))
    on = files_of(out)
    assert sorted(off) == [n for n in sorted(on) if not n.endswith('_grid.nc')] and len(on) == len(off) + 3
    assert all(on[n] == off[n] for n in off)


def test_run_ensemble_writes_the_maps(runs, tmp_path):
    """Two members, statistics = mean: a member's folder holds the files of the single run of its forcing, the maps byte
    for byte; ensemble/ holds the mean's map; overlapped and one after the other give the same bytes; member_outputs = 0
    writes no member maps."""
    from xanthos_amd import run_ensemble, synth
    w = runs.world
    got = {}
    for tag, overlap, member_outputs in (('overlapped', True, 1), ('serial', False, 1), ('statistics', True, 0)):
        root = str(tmp_path / tag)
        ini, _ = synth.write_ensemble_example(root, w, runs.forcings, 1971, 1973, runoff_spinup=25, routing_spinup=6,
                                              statistics=('mean',), statistics_vars=('q', 'avgchflow'), output_format=NPY,
                                              output_vars=VARS, gridded=True,
                                              member_outputs=member_outputs)
        run_ensemble(ini, overlap=overlap)
        out = os.path.join(root, 'output', PROJECT)
        assert sorted(os.listdir(out)) == ['ensemble', 'logfile.log'] + (['m00', 'm01'] if member_outputs else [])
        got[tag] = {d: files_of(os.path.join(out, d)) for d in sorted(os.listdir(out)) if d != 'logfile.log'}
    for k, member in enumerate(('m00', 'm01')):
        single = files_of(runs.out[k])
        assert sorted(got['overlapped'][member]) == sorted(single) and sum(n.endswith('_grid.nc') for n in single) == 3
        assert all(got['overlapped'][member][n] == single[n] for n in single), member
    ens = got['overlapped']['ensemble']
    stems = ['avgchflow_m3persec_{}_mean'.format(PROJECT), 'q_mmpermonth_{}_mean'.format(PROJECT)]
    assert sorted(ens) == sorted([s + '.npy' for s in stems] + [s + '_grid.nc' for s in stems])
    table = grid_np.cell_of_slot(w.coords, 36, 72)
    for s in stems:
        assert ens[s + '_grid.nc'].endswith(grid_np.grid_body(np.load(os.path.join(str(tmp_path), 'overlapped', 'output', PROJECT,
                                                                                    'ensemble', s + '.npy')), table).tobytes())
    assert got['serial'] == got['overlapped']
    assert got['statistics'] == {'ensemble': ens}
