"""The gridded output restated in numpy and scipy (tests/test_gridded_host.py, tests/test_gpu_gridded.py): which cell lies
in which slot, the body of a map as numpy forms it, and the same file written through scipy's netcdf_file."""
import datetime

import numpy as np

FILL_BITS = 0x7CF00000                                   # netCDF's NC_FILL_FLOAT
FILL = np.array([FILL_BITS], dtype='>u4').view('>f4')[0]
CF_UNITS = {'mmpermonth': 'mm month-1', 'km3permonth': 'km3 month-1', 'mmperyear': 'mm year-1',
            'km3peryear': 'km3 year-1', 'm3persec': 'm3 s-1'}


def slot_of_cell(coords, ncol):
    coords = np.asarray(coords)
    return (coords[:, 4].astype(np.int64) - 1) * ncol + coords[:, 3].astype(np.int64) - 1


def cell_of_slot(coords, nrow, ncol):
    """int32 [nrow * ncol]: the 0-based cell in every slot of the row-major grid, -1 where there is none."""
    table = np.full(nrow * ncol, -1, dtype=np.int32)
    table[slot_of_cell(coords, ncol)] = np.arange(len(coords), dtype=np.int32)
    return table


def grid_body(a, table):
    """[ncell, t] float64 -> [t, nslots] '>f4': the cells at their slots, the fill elsewhere and for NaN."""
    a = np.asarray(a, dtype=np.float64)
    table = np.asarray(table)
    slots = np.flatnonzero(table >= 0)
    at = np.empty(a.shape[0], dtype=np.int64)
    at[table[slots]] = slots                              # slot_of_cell
    g = np.full((a.shape[1], table.size), FILL, '>f4')
    with np.errstate(over='ignore'):
        v = a.T.astype('>f4')
    v[np.isnan(a.T)] = FILL
    g[:, at] = v
    return g


def time_days(start_year, nsteps, in_year):
    origin = datetime.date(start_year, 1, 1)
    return [(datetime.date(start_year + (k if in_year else k // 12), 1 if in_year else k % 12 + 1, 1) - origin).days
            for k in range(nsteps)]


def write_with_scipy(path, var, unit_str, days, start_year, lat, lon, body, title):
    """The file of gridded.grid_nc_header + body through scipy (which orders the variables by shape, not as the layout
    does: for reading back and comparing contents, not header bytes)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, 'w', version=1) as f:
        f.Conventions, f.title, f.source = 'CF-1.8', title, 'xanthos_amd'
        f.createDimension('time', len(days))
        f.createDimension('lat', len(lat))
        f.createDimension('lon', len(lon))
        t = f.createVariable('time', 'i4', ('time',))
        t[:] = days
        t.units, t.calendar = 'days since {:04d}-01-01 00:00:00'.format(start_year), 'proleptic_gregorian'
        t.standard_name, t.axis = 'time', 'T'
        y = f.createVariable('lat', 'f8', ('lat',))
        y[:] = lat
        y.units, y.standard_name, y.axis = 'degrees_north', 'latitude', 'Y'
        x = f.createVariable('lon', 'f8', ('lon',))
        x[:] = lon
        x.units, x.standard_name, x.axis = 'degrees_east', 'longitude', 'X'
        v = f.createVariable(var, 'f4', ('time', 'lat', 'lon'))
        v[:] = np.asarray(body).reshape(len(days), len(lat), len(lon))
        v.units, v.long_name = CF_UNITS[unit_str], var
        v._FillValue = v.missing_value = np.float32(FILL)


def contents(path):
    """What a reader sees: (dimensions in order, global attributes, {variable: (dimensions, attributes, bytes)})."""
    from scipy.io import netcdf_file
    with netcdf_file(path, mmap=False) as f:
        variables = {k: (v.dimensions, dict(v._attributes), v.data.dtype.str, v.data.tobytes()) for k, v in f.variables.items()}
        return list(f.dimensions.items()), dict(f._attributes), variables
