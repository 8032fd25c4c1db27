"""OutWriter for the hot-path outputs -- the array math of xanthos/data_writer/out_writer.py on the GPU.

Same constructor and methods as the reference class (:33-265): ``OutWriter(settings, grid_areas, all_outputs)``,
``write()``, ``get(var)``, ``write_aggregates(ref, values, basin, country, region)``.  Month -> year aggregation
(sum; mean for ``avgchflow``, :100-108), the mm -> km3 conversion (:111-112) and the basin / country / region sums
(:250-265) run as HIP kernels (csrc/xh_agg.hip, xh_diag.hip) on arrays that may already be resident in HBM, adding in
pandas' compensated order so that the values written equal the reference's bit for bit; only the (12x smaller
for yearly output) results cross PCIe.  Files are written as ``.csv`` (OutputFormat 1, the reference's layout:
an ``id`` column of 1-based cell ids and one column per time step), ``.npy`` (4), ``.nc`` (0: the NetCDF-classic file of
the reference's ``save_netcdf``, one 'f4' variable ``data``) or ``.mat`` (2: ``scipy.io.savemat``'s MAT-5 file of the
array); parquet (3) raises.  The csv text of a table without names is formatted in HBM as well (csrc/xh_csv.hip:
repr(float) per value, NaN the empty field) and only text crosses PCIe; the small tables with a ``name`` column (basin /
country / region sums) are written by the host loop.  NetCDF and MATLAB files are a header that depends on the shape and
the names alone (formats.py, made here) and a body formed in HBM (csrc/xh_pack.hip: big-endian binary32; xh_transpose:
column-major doubles) that leaves through the npy writer's path; the tables with names are cell arrays under MATLAB
(``savemat`` on the host), and NetCDF cannot hold them -- the reference fails there, this writer refuses the combination
when it is constructed.

With a ``grid`` (gridded.GridMap; [Project] GriddedOutput = 1) every per-cell table is written a second time as
``<same stem>_grid.nc``: a CF NetCDF map [time, lat, lon] of the array as written, its header made by gridded.py, its body
gathered, transposed and narrowed in HBM (csrc/xh_grid.hip).  The per-cell files are what they are without it.
"""
import logging
import os

import numpy as np

from .. import _hip
from ..ini_reader import ValidationException
from . import formats, gridded

FORMAT_NETCDF, FORMAT_CSV, FORMAT_MAT, FORMAT_PARQUET, FORMAT_NPY = 0, 1, 2, 3, 4
UNIT_MM_MTH, UNIT_KM3_MTH = 0, 1
NMONTHS = 12


class OutWriter:

    def __init__(self, settings, grid_areas, all_outputs, device=None, grid=None):
        # the reference's agg_spatial tables have a name column, which its save_netcdf cannot index (InvalidIndexError
        # after the whole run): refused before anything is computed for the writer
        aggregates = [k for k in ('AggregateRunoffBasin', 'AggregateRunoffCountry', 'AggregateRunoffGCAMRegion')
                      if getattr(settings, k, 0)]
        if settings.OutputFormat == FORMAT_NETCDF and aggregates:
            raise ValidationException(
                'OutputFormat = 0 (NetCDF) cannot hold the tables of {} = 1: they carry a name column, and the file has one '
                'float variable; use OutputFormat 1 (csv) or 2 (MATLAB), or switch the aggregation off'.format(
                    ' / '.join(aggregates)))
        self.output_names = [o for o in settings.output_vars if o in all_outputs.keys()]
        self.ctx = _hip.get_context(getattr(settings, 'device', 0) if device is None else device)
        self.inputs = {o: all_outputs[o] for o in self.output_names}           # host ndarray or DeviceArray
        self.outputs = [None] * len(self.output_names)
        # (the ensemble driver, ensemble.py) keep_device: the aggregated / converted arrays stay in HBM as well, for the
        # across-member statistics; write_files = False: the arrays are formed as written but no file is
        self.keep_device, self.write_files = False, True
        self.device_outputs = {}
        # lists while write() collects the files it flushes together
        self._npy_from_device = self._csv_from_device = self._bodies_from_device = self._grids_from_device = None
        self.grid = grid                                # gridded.GridMap: every per-cell table also as <stem>_grid.nc
        self.grid_areas = np.asarray(grid_areas, dtype=np.float64)
        self.conversion_mm_km3 = self.grid_areas / 1e6
        self.proj_name = settings.ProjectName
        self.out_folder = settings.OutputFolder
        self.out_format = settings.OutputFormat
        self.out_unit = settings.OutputUnit
        self.out_unit_str = '{}per{}'.format(('mm', 'km3')[settings.OutputUnit], ('month', 'year')[settings.OutputInYear])
        self.output_in_year = settings.OutputInYear
        years = range(settings.StartYear, settings.EndYear + 1)
        self.time_steps = ([str(y) for y in years] if self.output_in_year else
                           ['{}{:02}'.format(y, m) for y in years for m in range(1, NMONTHS + 1)])
        self.grid_time = gridded.time_axis(settings.StartYear, len(self.time_steps), self.output_in_year)
        if self.out_format not in (FORMAT_NETCDF, FORMAT_CSV, FORMAT_MAT, FORMAT_PARQUET, FORMAT_NPY):
            logging.warning('Output format {} is invalid; writing output as .csv'.format(self.out_format))
            self.out_format = FORMAT_CSV

    def get(self, varstr, host=True):
        """The written array of a variable (:77-79).  host=False may return the DeviceArray a monthly, unconverted
        variable was saved from."""
        i = self.output_names.index(varstr)
        if host and isinstance(self.outputs[i], _hip.DeviceArray):
            self.outputs[i] = self.outputs[i].download()
        return self.outputs[i]

    def get_device(self, varstr):
        """The written array of a variable in HBM, with keep_device: the aggregated / converted array write() kept, or the
        run's own array for a monthly, unconverted variable (which the next run overwrites); a host array is uploaded.
        Returns (DeviceArray, whether the caller owns it)."""
        if varstr in self.device_outputs:
            return self.device_outputs.pop(varstr), True
        a = self.inputs[varstr]
        if self.output_in_year or (self.out_unit == UNIT_KM3_MTH and varstr != 'avgchflow'):
            a = self.get(varstr)
        return (a, False) if isinstance(a, _hip.DeviceArray) else (self.ctx.upload(np.asarray(a, dtype=np.float64)), True)

    def unit_of(self, var):
        if var == 'drought_index':                      # (drought/standardized.py: a standard normal deviate)
            return '1'
        return 'm3persec' if var == 'avgchflow' else self.out_unit_str

    # ---- device helpers
    def _on_device(self, arr):
        if isinstance(arr, _hip.DeviceArray):
            return arr, False
        return self.ctx.upload(np.asarray(arr, dtype=np.float64)), True

    def _save_bodies(self, items):
        (self.ctx.save_nc_many if self.out_format == FORMAT_NETCDF else self.ctx.save_mat_many)(items)

    def agg_to_year(self, arr, func='sum', scale=None):
        """[ncell, nmonths] -> [ncell, nyears] (:237-248), optionally x scale[c] afterwards. Returns a host array."""
        return self._agg(arr, NMONTHS, 0 if func == 'sum' else 1, scale)

    def _agg(self, arr, group, mode, scale, keep=None, on_device=False):
        """on_device: the result stays in HBM and is returned as a DeviceArray (the csv writer formats it there)."""
        src, mine = self._on_device(arr)
        ncell, ncols = src.shape
        dst = self.ctx.empty((ncell, ncols // group))
        d_scale = None if scale is None else self.ctx.upload(scale)
        self.ctx.agg_time(ncell, ncols, group, mode, d_scale, src, dst)
        out = dst if on_device else dst.download()
        if keep is not None and self.keep_device:
            self.device_outputs[keep], dst = dst, None
        for b in (None if on_device else dst, d_scale, src if mine else None):
            if b is not None:
                b.free()
        return out

    def agg_spatial(self, arr, id_map, n_ids, first_id=1):
        """[ncell, t] -> [n_ids, t]: per id, pandas' compensated NaN-skipping sum over its cells in ascending order
        (groupby('id').sum(), :250-265) on xh_diag_group_sum; ids first_id .. first_id + n_ids - 1, the others dropped;
        an id without cells gives NaN (the left merge of the names)."""
        src, mine = self._on_device(arr)
        ncell, ncols = src.shape
        idx = np.asarray(id_map).reshape(-1).astype(np.int64) - first_id
        if idx.shape != (ncell,):
            raise ValueError('the id map holds {} cells, the data {}'.format(idx.shape[0], ncell))
        idx[(idx < 0) | (idx >= n_ids)] = -1
        dst, d_counts = self.ctx.empty((n_ids, ncols)), self.ctx.empty((n_ids,), dtype=np.int64)
        self.ctx.diag_group_sum(ncell, ncols, n_ids, idx, src, dst, d_counts)
        out, counts = dst.download(), d_counts.download()
        for b in (dst, d_counts, src if mine else None):
            if b is not None:
                b.free()
        out[counts == 0] = np.nan
        return out

    # ---- the reference's write() (:81-125)
    def write(self):
        if not self.output_names:
            logging.debug('No valid output variables specified')
            return
        self._npy_from_device = []                      # monthly, unconverted npy outputs still in HBM: saved side by side
        self._csv_from_device = []                      # csv outputs: formatted in HBM and written side by side
        self._bodies_from_device = []                   # NetCDF / MATLAB outputs: bodies formed in HBM, written side by side
        self._grids_from_device = []                    # the maps next to them (grid): the same
        # csv: an aggregated / converted array stays in HBM for the formatter (get() fetches it on demand); with keep_device
        # that array goes to the caller afterwards, so the host copy is made here as before
        # (NetCDF / MATLAB: the same, for the kernels that form the file's body)
        lazy = self.out_format in (FORMAT_CSV, FORMAT_NETCDF, FORMAT_MAT) and self.write_files and not self.keep_device
        for i, var in enumerate(self.output_names):
            flow = var == 'avgchflow'
            unit = 'm3persec' if flow else self.out_unit_str
            scale = self.conversion_mm_km3 if (self.out_unit == UNIT_KM3_MTH and not flow) else None
            if self.output_in_year:
                self.outputs[i] = self._agg(self.inputs[var], NMONTHS, 1 if flow else 0, scale, keep=var, on_device=lazy)
            elif scale is not None:
                self.outputs[i] = self._agg(self.inputs[var], 1, 0, scale, keep=var, on_device=lazy)
            else:
                a = self.inputs[var]
                # a device array is saved (npy, NetCDF, MATLAB) or formatted (csv) from HBM
                keep = isinstance(a, _hip.DeviceArray) and self.out_format != FORMAT_PARQUET
                if not self.write_files:
                    self.outputs[i] = a
                    continue
                self.outputs[i] = a if keep else (a.download() if isinstance(a, _hip.DeviceArray) else np.asarray(a))
            if not self.write_files:
                continue
            filename = os.path.join(self.out_folder, '{}_{}_{}'.format(var, unit, self.proj_name))
            data = self.outputs[i]
            if self.out_format in (FORMAT_CSV, FORMAT_NETCDF, FORMAT_MAT):      # the array as written that is in HBM already, if any
                data = self.device_outputs.get(var, data)
            self.write_data(filename, var, data, self.time_steps, first_id=1)
        if self._npy_from_device:
            self.ctx.save_npy_many(self._npy_from_device)
        if self._csv_from_device:
            self.ctx.csv_write_many([item for item, _ in self._csv_from_device])
            for (_, dev, _, _), mine in self._csv_from_device:
                if mine:
                    dev.free()
        if self._bodies_from_device:
            self._save_bodies([item for item, _ in self._bodies_from_device])
            for (_, _, dev), mine in self._bodies_from_device:
                if mine:
                    dev.free()
        if self._grids_from_device:
            self.ctx.save_grid_nc_many([item for item, _ in self._grids_from_device])
            for (_, _, dev, _), mine in self._grids_from_device:
                if mine:
                    dev.free()
        self._npy_from_device = self._csv_from_device = self._bodies_from_device = self._grids_from_device = None

    def write_aggregates(self, ref, values, basin, country, region):
        """Spatial sums of ``values`` (the written runoff) by basin / country / GCAM region (:126-158).

        As in the reference's ``agg_spatial`` (:250-265) there is one row per NAME: basins and regions are numbered from
        1 (``inc_name_idx=True``), countries from 0 (the names table keeps its 0-based index there); ids without a
        name are dropped, names without cells give NaN.  The csv carries the ``id`` and ``name`` columns the
        reference's DataFrame has."""
        filepath = os.path.join(self.out_folder, '{}_' + '{}_{}'.format(self.out_unit_str, self.proj_name))
        jobs = []
        if basin:
            names = getattr(ref, 'basin_names', None)
            n = len(names) if names is not None else getattr(ref, 'n_basin_names', int(np.max(ref.basin_ids)))
            jobs.append(('Basin_runoff', ref.basin_ids, n, 1, names))
        if country:
            if getattr(ref, 'country_ids', None) is None:
                raise ValueError('AggregateRunoffCountry needs country ids and names (country.csv, country-names.csv)')
            jobs.append(('Country_runoff', ref.country_ids, len(ref.country_names), 0, ref.country_names))
        if region:
            if getattr(ref, 'region_ids', None) is None:
                raise ValueError('AggregateRunoffGCAMRegion needs region ids and names (region32_grids.csv, '
                                 'Rgn32Names.csv)')
            jobs.append(('GCAMRegion_runoff', ref.region_ids, len(ref.region_names), 1, ref.region_names))
        out = {}
        for name, ids, n, first, names in jobs:
            logging.info('Aggregating by ' + name.split('_')[0])
            out[name] = self.agg_spatial(values, ids, n, first_id=first)
            self.write_data(filepath.format(name), name, out[name], self.time_steps, first_id=first, names=names)
        logging.info('Aggregated unit is {}'.format(self.out_unit_str))
        return out

    def write_data(self, filename, var, data, col_names, first_id=1, names=None):
        self._write_table(filename, var, data, col_names, first_id, names)
        if self.grid is not None and names is None and data.shape[0] == self.grid.ncell and self.write_files:
            self._write_grid(filename, var, data)

    def _write_grid(self, filename, var, data):
        """``<filename>_grid.nc``: the per-cell table ``data`` as a map [time, lat, lon] (gridded.py), from its copy in HBM
        where there is one."""
        collect = self._grids_from_device is not None and var in self.output_names
        if collect:                                     # (write() under keep_device: the array as written is in HBM as well)
            data = self.device_outputs.get(var, data)
        days, units = self.grid_time
        header = gridded.grid_nc_header(var, self.unit_of(var), days[:data.shape[1]], units, self.grid, title=self.proj_name)
        dev, mine = self._on_device(data)
        item = (filename + '_grid.nc', header, dev, self.grid)
        if collect:
            self._grids_from_device.append((item, mine))                         # flushed at the end of write()
        else:
            self.ctx.save_grid_nc_many([item])
            if mine:
                dev.free()

    def _write_table(self, filename, var, data, col_names, first_id, names):
        os.makedirs(self.out_folder, exist_ok=True)
        if self.out_format == FORMAT_NPY:
            if isinstance(data, _hip.DeviceArray):
                if self._npy_from_device is not None and var in self.output_names:
                    self._npy_from_device.append((filename + '.npy', data))      # flushed at the end of write()
                else:
                    self.ctx.save_npy(filename + '.npy', data)
            else:
                np.save(filename + '.npy', data)
        elif self.out_format == FORMAT_CSV and names is None:
            # the lines are formatted in HBM (xh_csv_write): header here, the text of the table behind it
            dev, mine = self._on_device(data)
            with open(filename + '.csv', 'w') as fh:
                fh.write('id,' + ','.join(col_names[:dev.shape[1]]) + '\n')
                item = (filename + '.csv', dev, first_id, fh.tell())
            if self._csv_from_device is not None and var in self.output_names:
                self._csv_from_device.append((item, mine))                       # flushed at the end of write()
            else:
                self.ctx.csv_write(*item)
                if mine:
                    dev.free()
        elif self.out_format == FORMAT_CSV:             # a table with names (a few hundred rows): the host loop
            ids = np.arange(first_id, first_id + data.shape[0])
            header = 'id,' + ('name,' if names is not None else '') + ','.join(col_names[:data.shape[1]])
            fmt = lambda v: '' if v != v else repr(float(v))                    # pandas writes NaN as an empty field
            with open(filename + '.csv', 'w') as fh:
                fh.write(header + '\n')
                for k, (i, row) in enumerate(zip(ids, data)):
                    label = '' if names is None else str(names[k]) + ','
                    fh.write(str(i) + ',' + label + ','.join(fmt(v) for v in row) + '\n')
        elif self.out_format == FORMAT_MAT and names is not None:      # a table with names: a cell array, on the host
            formats.save_mat_table(filename + '.mat', var, data, names)
        elif self.out_format in (FORMAT_NETCDF, FORMAT_MAT):
            # the header here, the body formed in HBM behind it (xh_pack_f32_be / xh_transpose)
            nc = self.out_format == FORMAT_NETCDF
            if names is not None:
                raise ValidationException('OutputFormat = 0 (NetCDF) cannot hold table {} with its name column'.format(var))
            nrows, ncols = data.shape
            header = (formats.nc_header(nrows, ncols, self.output_in_year, self.out_unit_str, var) if nc else
                      formats.mat_header(var, nrows, ncols))
            dev, mine = self._on_device(data)
            item = (filename + ('.nc' if nc else '.mat'), header, dev)
            if self._bodies_from_device is not None and var in self.output_names:
                self._bodies_from_device.append((item, mine))                    # flushed at the end of write()
            else:
                self._save_bodies([item])
                if mine:
                    dev.free()
        else:
            raise RuntimeError('OutputFormat 3 (parquet) is not written: the reference needs fastparquet for it; use 0 '
                               '(NetCDF), 1 (csv), 2 (MATLAB) or 4 (npy)')
