"""Host side of the gridded output (no GPU): GridMap against the restatement of tests/grid_np.py and its refusals,
grid_nc_header read back through scipy and through nc_header.variable_range, the [Project] GriddedOutput key."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_np  # noqa: E402

from xanthos_amd import synth  # noqa: E402
from xanthos_amd.data_writer import gridded  # noqa: E402
from xanthos_amd.ini_reader import ConfigReader, ValidationException  # noqa: E402

NROW, NCOL = 36, 72


@pytest.fixture(scope='module')
def world():
    return synth.make_world(nrow=NROW, ncol=NCOL, ncell=900, n_basins=7, seed=12)


# ---- GridMap
def test_map_equals_the_restatement(world):
    g = gridded.GridMap(world.coords, NROW, NCOL)
    table = grid_np.cell_of_slot(world.coords, NROW, NCOL)
    assert g.cell_of_slot.dtype == np.int32 and g.cell_of_slot.shape == (NROW * NCOL,) == (g.nslots,)
    assert np.array_equal(g.cell_of_slot, table) and (table >= 0).sum() == 900 == g.ncell
    assert np.array_equal(g.slot_of_cell, grid_np.slot_of_cell(world.coords, NCOL))
    assert not (np.diff(g.slot_of_cell) > 0).all()              # the table is column-major: cell order is not slot order
    # the synthetic world counts rows from the south; rows without a cell (the margins) get the fitted value
    assert np.abs(g.lat - (-90 + (np.arange(NROW) + .5) * 180 / NROW)).max() <= 1e-9
    assert np.abs(g.lon - (-180 + (np.arange(NCOL) + .5) * 360 / NCOL)).max() <= 1e-9
    assert g.fill_bits == grid_np.FILL_BITS == 0x7CF00000


def test_a_north_first_table_gives_a_descending_lat(world):
    coords = world.coords.copy()
    coords[:, 4] = NROW + 1 - coords[:, 4]
    g = gridded.GridMap(coords, NROW, NCOL)
    assert (np.diff(g.lat) < 0).all() and np.abs(g.lat - (90 - (np.arange(NROW) + .5) * 180 / NROW)).max() <= 1e-9
    assert np.array_equal(g.cell_of_slot, grid_np.cell_of_slot(coords, NROW, NCOL))


def test_a_grid_of_one_row_needs_no_fit():
    coords = np.array([[1, 10.0, 5.0, 1, 1], [2, 30.0, 5.0, 3, 1]])
    g = gridded.GridMap(coords, 1, 3)
    assert list(g.cell_of_slot) == [0, -1, 1] and list(g.lat) == [5.0] and list(g.lon) == [10.0, 20.0, 30.0]


def _edited(world, cell, column, value):
    coords = world.coords.copy()
    coords[cell, column] = value
    return coords


@pytest.mark.parametrize('edit,match', [
    (lambda w: _edited(w, 17, 3, w.coords[17, 3] + 0.5), 'cell 18 .*not an integer'),
    (lambda w: _edited(w, 17, 4, np.nan), 'cell 18 .*not an integer'),
    (lambda w: _edited(w, 40, 4, NROW + 1), 'cell 41 .*outside 1..36'),
    (lambda w: _edited(w, 40, 3, 0), 'cell 41 .*outside 1..72'),
    (lambda w: np.vstack([w.coords, [[901] + list(w.coords[5, 1:])]]), 'cell 6 .*shares its slot .*with cell 901'),
    (lambda w: _edited(w, 99, 2, w.coords[99, 2] + 1e-6), 'cell 100 .*off the row axis'),
    (lambda w: _edited(w, 99, 1, w.coords[99, 1] - 1e-6), 'cell 100 .*off the column axis'),
    (lambda w: w.coords[w.coords[:, 4] == w.coords[0, 4]], 'cell [0-9]+ .*fewer than two distinct rows'),
    (lambda w: w.coords[w.coords[:, 3] == w.coords[0, 3]], 'cell [0-9]+ .*fewer than two distinct columns'),
], ids=['half-index', 'nan-index', 'row-outside', 'column-outside', 'two-in-one-slot', 'lat-off', 'lon-off', 'one-row',
        'one-column'])
def test_refusals_name_the_cell(world, edit, match):
    with pytest.raises(ValidationException, match=match):
        gridded.GridMap(edit(world), NROW, NCOL)


# ---- the file
@pytest.mark.parametrize('start,in_year,nsteps', [(1899, 0, 36), (2099, 0, 24), (1898, 1, 5), (1971, 0, 36)],
                         ids=['over-1900', 'over-2100', 'years-over-1900', 'plain'])
def test_header_and_body_read_back(world, tmp_path, start, in_year, nsteps):
    """1900 and 2100 are leap years by the model's year % 4 rule and not by the calendar: the time axis is the calendar's."""
    g = gridded.GridMap(world.coords, NROW, NCOL)
    rng = np.random.default_rng(start)
    a = rng.standard_normal((900, nsteps)) * 100
    a[5, 1 % nsteps] = np.nan
    unit = 'mmperyear' if in_year else 'km3permonth'
    days, units = gridded.time_axis(start, nsteps, in_year)
    assert list(days) == grid_np.time_days(start, nsteps, in_year) and units == 'days since {}-01-01 00:00:00'.format(start)
    if not in_year and start in (1899, 2099):
        assert days[12 + 2] - days[12 + 1] == 28                # February 1900 / 2100
    header = gridded.grid_nc_header('q', unit, days, units, g, title='proj')
    assert header == gridded.grid_nc_header('q', unit, days.copy(), units, gridded.GridMap(world.coords, NROW, NCOL), title='proj')
    body = grid_np.grid_body(a, g.cell_of_slot)
    assert body.shape == (nsteps, g.nslots) and body.dtype == np.dtype('>f4')
    path, ref = str(tmp_path / 'q_grid.nc'), str(tmp_path / 'scipy.nc')
    with open(path, 'wb') as fh:
        fh.write(header + body.tobytes())
    dims, glob, variables = grid_np.contents(path)
    assert dims == [('time', nsteps), ('lat', NROW), ('lon', NCOL)]
    assert glob == {'Conventions': b'CF-1.8', 'title': b'proj', 'source': b'xanthos_amd'}
    assert list(variables) == ['time', 'lat', 'lon', 'q']       # the data variable last: its body ends the file
    grid_np.write_with_scipy(ref, 'q', unit, grid_np.time_days(start, nsteps, in_year), start, g.lat, g.lon, body, 'proj')
    r_dims, r_glob, r_variables = grid_np.contents(ref)
    assert sorted(dims) == sorted(r_dims) and glob == r_glob and sorted(variables) == sorted(r_variables)
    for name, (vdims, atts, dtype, raw) in variables.items():
        assert (vdims, dtype, raw) == (r_variables[name][0], r_variables[name][2], r_variables[name][3]), name
        assert atts.keys() == r_variables[name][1].keys(), name
        for k, v in atts.items():
            r = r_variables[name][1][k]
            assert (v == r and type(v) is type(r)) if isinstance(v, bytes) else (
                np.asarray(v).dtype == np.float32 and np.asarray(v).tobytes() == np.asarray(r).tobytes()), (name, k)
    assert variables['q'][0] == ('time', 'lat', 'lon') and variables['q'][3] == body.tobytes()
    assert variables['q'][1]['units'] == grid_np.CF_UNITS[unit].encode()
    fill = np.asarray(variables['q'][1]['_FillValue'], dtype='>f4').tobytes()
    assert fill == np.asarray(variables['q'][1]['missing_value'], dtype='>f4').tobytes() == bytes([0x7C, 0xF0, 0, 0])
    # a NaN in a land cell and every slot without a cell hold the fill
    cube = np.frombuffer(variables['q'][3], '>u4').reshape(nsteps, -1)
    assert (cube[:, g.cell_of_slot < 0] == grid_np.FILL_BITS).all() and cube[1 % nsteps, g.slot_of_cell[5]] == grid_np.FILL_BITS
    assert (cube[:, g.cell_of_slot >= 0] != grid_np.FILL_BITS).sum() == 900 * nsteps - 1
    from xanthos_amd.nc_header import variable_range
    assert variable_range(path, 'q') == (np.dtype('>f4'), (nsteps, NROW, NCOL), len(header))
    assert variable_range(path, 'lat')[:2] == (np.dtype('>f8'), (NROW,))


@pytest.mark.parametrize('unit', sorted(grid_np.CF_UNITS))
def test_units_are_cf_style(world, tmp_path, unit):
    g = gridded.GridMap(world.coords, NROW, NCOL)
    days, units = gridded.time_axis(1971, 1, 0)
    path = str(tmp_path / 'u.nc')
    with open(path, 'wb') as fh:
        fh.write(gridded.grid_nc_header('avgchflow', unit, days, units, g) + grid_np.grid_body(np.zeros((900, 1)), g.cell_of_slot).tobytes())
    assert grid_np.contents(path)[2]['avgchflow'][1]['units'] == grid_np.CF_UNITS[unit].encode()


def test_two_gib_are_refused():
    """360 x 720 slots x 4 bytes x 2072 months reach 2^31; 2071 do not (the header alone is formed: no cube)."""
    coords = np.array([[1, -179.75, -89.75, 1, 1], [2, 179.75, 89.75, 720, 360]])
    g = gridded.GridMap(coords, 360, 720)
    days, units = gridded.time_axis(1850, 2072, 0)
    assert 2072 * g.nslots * 4 >= 1 << 31 > 2071 * g.nslots * 4
    with pytest.raises(ValidationException, match="cannot hold variable 'q'.*limit is 2 GiB per variable; use OutputInYear = 1"):
        gridded.grid_nc_header('q', 'mmpermonth', days, units, g)
    assert len(gridded.grid_nc_header('q', 'mmpermonth', days[:2071], units, g)) > 2071 * 4 + 1080 * 8


# ---- the key
@pytest.fixture
def ini(tmp_path):
    w = synth.make_world(nrow=36, ncol=72, ncell=200, n_basins=3, seed=2)
    return lambda **kw: synth.write_example(str(tmp_path), w, synth.make_forcing(w, 24), 1971, 1972, runoff_spinup=12, **kw)


def test_the_key(ini):
    plain = ini()
    assert 'GriddedOutput' not in open(plain).read() and ConfigReader(plain).GriddedOutput == 0
    on = ini(gridded=True)
    text = open(on).read()
    assert 'GriddedOutput = 1' in text and ConfigReader(on).GriddedOutput == 1
    assert text.replace('GriddedOutput = 1\n', '') == open(ini()).read()      # nothing else changes in the example
    for bad in ('2', '-1', 'yes', '1.0'):
        with open(on, 'w') as fh:
            fh.write(text.replace('GriddedOutput = 1', 'GriddedOutput = ' + bad))
        with pytest.raises(ValidationException, match='GriddedOutput must be 0 or 1'):
            ConfigReader(on)
