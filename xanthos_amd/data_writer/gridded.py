"""Gridded CF NetCDF maps ``[time, lat, lon]`` of the per-cell outputs ([Project] GriddedOutput = 1).

The reference writes per-cell tables only: ``[ncell, t]`` rows in the order of ``coordinates.csv``.  A viewer or a GIS wants
a map: time-major, longitude fastest, coordinate variables, a fill value where no cell lies.  Two things are made here,
both on the host and both small:

* ``GridMap``: which cell lies in which slot of the ``ngridrow x ngridcol`` grid (``slot = (ilat - 1) * ngridcol + ilon -
  1`` from the loader's coordinates table), validated, and the ``lat`` / ``lon`` axes fitted from the cells' own coordinates;
* ``grid_nc_header``: the bytes of a NetCDF-classic (CDF-1) file in front of the data variable's body -- dimensions,
  CF attributes and the three coordinate variables' values -- a pure function like ``formats.nc_header``.

The body, ``[ncols, nslots]`` big-endian binary32, is gathered, transposed and narrowed in HBM (csrc/xh_grid.hip,
``Context.save_grid_nc_many``) from the array as written and leaves behind the header through the npy writer's path.
"""
import datetime
import struct

import numpy as np

from ..ini_reader import ValidationException
from .formats import NC_LIMIT, _NC_ATTRIBUTE, _NC_DIMENSION, _NC_FLOAT, _NC_VARIABLE, _nc_int, _nc_string, \
    _nc_text_attribute

FILL_BITS = 0x7CF00000                   # netCDF's default float fill, NC_FILL_FLOAT (about 9.96921e36)
FILL = np.array([FILL_BITS], dtype=np.uint32).view(np.float32)[0]
AXIS_TOLERANCE = 1e-9                    # degrees a cell's lat / lon may lie off the fitted axis
CF_UNITS = {'mmpermonth': 'mm month-1', 'km3permonth': 'km3 month-1', 'mmperyear': 'mm year-1',
            'km3peryear': 'km3 year-1', 'm3persec': 'm3 s-1'}
_NC_INT, _NC_DOUBLE = 4, 6


def _refuse(cell_id, why):
    return ValidationException('GriddedOutput = 1: cell {} of the coordinates table {}'.format(int(cell_id), why))


def _fit_axis(ids, index, value, n, what):
    """value = a + b * (index - 1) through the cells' own coordinates; the axis [n] of the fitted values."""
    lo, hi = int(np.argmin(index)), int(np.argmax(index))
    if index[lo] == index[hi]:
        if n != 1:
            raise _refuse(ids[lo], 'and every other cell lie in one {0}: the {0} axis of {1} cannot be fitted from fewer than '
                          'two distinct {0}s'.format(what, n))
        a, b = float(value[lo]), 0.0
    else:
        b = (float(value[hi]) - float(value[lo])) / float(index[hi] - index[lo])
        a = float(value[lo]) - b * float(index[lo] - 1)
    off = np.abs(value - (a + b * (index - 1)))
    bad = int(np.argmax(off))
    if not off[bad] <= AXIS_TOLERANCE:       # (a NaN coordinate fails too)
        raise _refuse(ids[bad], 'lies {:.3g} degrees off the {} axis fitted from the table ({} + {} per index)'.format(
            float(off[bad]), what, a, b))
    return a + b * np.arange(n, dtype=np.float64)


class GridMap:
    """Cells of the coordinates table ``[id, lon, lat, ilon, ilat]`` (1-based indices) on the ``ngridrow x ngridcol`` grid.

    ``slot_of_cell`` [ncell] int64, ``cell_of_slot`` [nslots] int32 (-1: no cell), ``lat`` [ngridrow], ``lon`` [ngridcol] in
    whatever direction the table counts its rows and columns."""

    fill_bits = FILL_BITS

    def __init__(self, coords, ngridrow, ngridcol):
        coords = np.asarray(coords, dtype=np.float64)
        if coords.ndim != 2 or coords.shape[1] < 5 or coords.shape[0] < 1:
            raise ValidationException('GriddedOutput = 1 needs the coordinates table [id, lon, lat, ilon, ilat]')
        self.ngridrow, self.ngridcol = int(ngridrow), int(ngridcol)
        self.nslots, self.ncell = self.ngridrow * self.ngridcol, coords.shape[0]
        ids, lon, lat, ilon, ilat = (coords[:, k] for k in range(5))
        for index, n, what in ((ilat, self.ngridrow, 'ilat'), (ilon, self.ngridcol, 'ilon')):
            whole = index == np.floor(index)                   # (NaN and inf fail)
            if not whole.all():
                k = int(np.argmin(whole))
                raise _refuse(ids[k], 'has {} = {}, which is not an integer'.format(what, index[k]))
            inside = (index >= 1) & (index <= n)
            if not inside.all():
                k = int(np.argmin(inside))
                raise _refuse(ids[k], 'has {} = {} outside 1..{}'.format(what, int(index[k]), n))
        self.slot_of_cell = (ilat.astype(np.int64) - 1) * self.ngridcol + (ilon.astype(np.int64) - 1)
        self.cell_of_slot = np.full(self.nslots, -1, dtype=np.int32)
        self.cell_of_slot[self.slot_of_cell] = np.arange(self.ncell, dtype=np.int32)
        twice = self.cell_of_slot[self.slot_of_cell] != np.arange(self.ncell)
        if twice.any():                                        # the later cell of a slot won the assignment above
            k = int(np.argmax(twice))
            raise _refuse(ids[k], 'shares its slot (ilat {}, ilon {}) with cell {}'.format(
                int(ilat[k]), int(ilon[k]), int(ids[self.cell_of_slot[self.slot_of_cell[k]]])))
        self.lat = _fit_axis(ids, ilat, lat, self.ngridrow, 'row')
        self.lon = _fit_axis(ids, ilon, lon, self.ngridcol, 'column')
        self._device = None

    def device_table(self, ctx):
        """``cell_of_slot`` in HBM: uploaded once (by ``ctx``) and kept.  Kernels take pointers only, so another context of
        the same device may use the copy (the ensemble's writing context)."""
        if self._device is None or self._device.ptr is None:
            self._device = ctx.upload(self.cell_of_slot, dtype=np.int32)
        return self._device


def time_axis(start_year, nsteps, in_year):
    """(days since <start_year>-01-01 of the first day of every month, or of every year with ``in_year``, by the real
    calendar; the CF units string)."""
    origin = datetime.date(int(start_year), 1, 1)
    if in_year:
        days = [(datetime.date(int(start_year) + k, 1, 1) - origin).days for k in range(int(nsteps))]
    else:
        days = [(datetime.date(int(start_year) + k // 12, k % 12 + 1, 1) - origin).days for k in range(int(nsteps))]
    return np.asarray(days, dtype=np.int64), 'days since {:04d}-01-01 00:00:00'.format(int(start_year))


def _attributes(pairs):
    """An attribute list: text values, or (nc_type, packed big-endian bytes of ONE value)."""
    out = _nc_int(_NC_ATTRIBUTE) + _nc_int(len(pairs))
    for name, value in pairs:
        if isinstance(value, str):
            out += _nc_text_attribute(name, value)
        else:
            nc_type, raw = value
            out += _nc_string(name) + _nc_int(nc_type) + _nc_int(1) + raw + b'\x00' * (-len(raw) % 4)
    return out


def grid_nc_header(var, unit_str, time_values, time_units, grid, title=''):
    """The bytes of ``<stem>_grid.nc`` in front of the body of variable ``var``: NetCDF classic (CDF-1), no record
    dimension; dimensions time, lat, lon; the global attributes Conventions = "CF-1.8", title, source (no date, no history:
    two runs give the same bytes); the variables time (i4), lat (f8), lon (f8) with their values, and ``var`` (f4 over
    [time, lat, lon]; units, long_name, _FillValue, missing_value) LAST, so that the returned bytes end where its
    ``len(time_values) * grid.nslots`` big-endian binary32 values begin."""
    time_values = np.asarray(time_values)
    nt = int(time_values.shape[0])
    vsize = nt * grid.nslots * 4                               # a multiple of 4: no padding behind the data
    if vsize >= NC_LIMIT:
        raise ValidationException(
            "GriddedOutput = 1 (NetCDF classic) cannot hold variable '{}': {} x {} x {} values are {} bytes, the format's "
            'limit is 2 GiB per variable; use OutputInYear = 1'.format(var, nt, grid.ngridrow, grid.ngridcol, vsize))
    fill = struct.pack('>I', FILL_BITS)
    head = b'CDF\x01' + _nc_int(0)                             # no records
    head += _nc_int(_NC_DIMENSION) + _nc_int(3)
    head += _nc_string('time') + _nc_int(nt) + _nc_string('lat') + _nc_int(grid.ngridrow)
    head += _nc_string('lon') + _nc_int(grid.ngridcol)
    head += _attributes([('Conventions', 'CF-1.8'), ('title', str(title)), ('source', 'xanthos_amd')])
    bodies = (time_values.astype('>i4').tobytes(), np.asarray(grid.lat).astype('>f8').tobytes(),
              np.asarray(grid.lon).astype('>f8').tobytes())
    variables = [
        ('time', [0], _attributes([('units', time_units), ('calendar', 'proleptic_gregorian'),
                                   ('standard_name', 'time'), ('axis', 'T')]), _NC_INT, len(bodies[0])),
        ('lat', [1], _attributes([('units', 'degrees_north'), ('standard_name', 'latitude'), ('axis', 'Y')]),
         _NC_DOUBLE, len(bodies[1])),
        ('lon', [2], _attributes([('units', 'degrees_east'), ('standard_name', 'longitude'), ('axis', 'X')]),
         _NC_DOUBLE, len(bodies[2])),
        (var, [0, 1, 2], _attributes([('units', CF_UNITS.get(unit_str, unit_str)), ('long_name', var),
                                      ('_FillValue', (_NC_FLOAT, fill)), ('missing_value', (_NC_FLOAT, fill))]),
         _NC_FLOAT, vsize)]
    # every entry ends in vsize and begin (4 bytes each): the header's length is known before the offsets are
    entries = [_nc_string(name) + _nc_int(len(dims)) + b''.join(_nc_int(d) for d in dims) + atts + _nc_int(nc_type)
               for name, dims, atts, nc_type, _ in variables]
    head += _nc_int(_NC_VARIABLE) + _nc_int(len(variables))
    begin = len(head) + sum(len(e) + 8 for e in entries)
    for entry, (_, _, _, _, size) in zip(entries, variables):
        padded = size + (-size % 4)
        head += entry + _nc_int(padded) + _nc_int(begin)
        begin += padded
    for raw in bodies:
        head += raw + b'\x00' * (-len(raw) % 4)
    return head
