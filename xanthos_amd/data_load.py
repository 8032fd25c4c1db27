"""Input loading for the pm / abcd / mrtm path (host side, runs once).

Mirrors the parts of xanthos/data_reader/data_load.py that feed the hot path and keeps every load-time transform that
changes its inputs:

* area x 0.01 (ha -> km2, :48); coordinates table [id, lon, lat, ilon, ilat] (:51); basin ids (:54)
* PM forcings pass through nan_to_num (:120-125) -- on the device after upload (``xh_nan_to_num``), on the host only if
  ``settings.device_transforms = False``; ``tairprev`` is tas shifted by one CELL, zeros for cell 0 (:127-129);
  land cover and elevation nan_to_num (:132,:135); 13 per-class parameters + 4 per-(class, month) tables (:94-117)
* precipitation keeps NaN (:186); ABCD tmin nan_to_num (:194-195), optional
* Hargreaves: temperature and daily temperature range as loaded (the kernel clamps and cleans them), latitude in
  radians (:71-84); GWAM: the maximum-soil-moisture composite with the water bodies and the initial soil moisture
  (:149-182, :226-260)
* Hargreaves-Samani: tas, tmin and tmax as loaded, NaN kept (:86-90); Thornthwaite: tas through nan_to_num (:137-138),
  on the device after upload unless ``device_transforms = False``
* diagnostics: the four comparison tables as loaded (:216-220)
* forcing stored as float32 or as a NetCDF-classic `float` / `double` variable stays AS STORED (a read-only map of the
  file) when the run reads it only through ``DevicePipeline.set_forcing`` -- the stored bytes cross PCIe and ``xh_widen``
  makes the doubles in HBM, exactly ``astype(float64)``; every other run gets float64 here (``DataLoader.keeps_stored``)
* routing: flow distance < 1000 -> 1000 (:204-205), velocity < 0 -> 0 (:207-208), 2-D DRT maps flattened with the
  reference's ``vectorize`` (:415-425), zero initial channel storage in historic mode (:427-438)

Any setting may be an in-memory ndarray instead of a path (data_load.py:305-307), which is how tests and benchmarks
inject synthetic forcing.
"""
import os

import numpy as np

from .ini_reader import ValidationException


def load_file(fn, header_num=0, key=None, mmap=False):
    """.npy / .csv / .txt / .nc (NetCDF classic) / .mat reader, same dispatch as data_load.py:342-390.
    mmap: a .npy comes back as a read-only memory map (np.load(mmap_mode='r')): nothing is read until someone looks, and
    the pipeline sends the file's bytes to the GPU itself (xh_upload_file).  So does a `float` or `double` variable of a
    .nc that is one block of the file (nc_header.variable_range): a read-only map of its big-endian values, as stored."""
    if isinstance(fn, np.ndarray):
        return fn
    if not os.path.isfile(fn):
        raise IOError('Error: File does not exist:', fn)
    if fn.endswith('.npy'):
        return np.load(fn, mmap_mode='r' if mmap else None)
    if fn.endswith('.mat'):
        import scipy.io as sio
        return sio.loadmat(fn)[key]
    if fn.endswith('.nc'):
        if mmap:
            from .nc_header import variable_range
            where = variable_range(fn, key)
            if where is not None:
                return np.memmap(fn, dtype=where[0], mode='r', offset=where[2], shape=where[1])
        import scipy.io as sio
        grp = sio.netcdf_file(fn, 'r', mmap=False)
        data = grp.variables[key][:].copy()
        grp.close()
        if data.dtype.byteorder == '>':            # NetCDF classic is big-endian (data_load.py:381-384)
            data = data.byteswap().view(data.dtype.newbyteorder())
        return data
    if fn.endswith('.csv') or fn.endswith('.txt'):
        delim = ',' if fn.endswith('.csv') else ' '
        try:            # numpy's C tokenizer: ~15x faster than genfromtxt on the 67,420-row grid tables; same values
            return np.loadtxt(fn, delimiter=delim, skiprows=header_num, dtype=float)
        except ValueError:      # missing fields (the reference fills them with 0), ragged or non-numeric columns
            return np.genfromtxt(fn, delimiter=delim, skip_header=header_num, filling_values='0')
    raise RuntimeError('File {} has unrecognized extension'.format(fn))


def stored_kind(arr):
    """(xh_widen kind, label) of a forcing array that may cross PCIe as it is stored -- a C-contiguous 2-D ndarray or
    memory map of float32, big-endian float32 or big-endian float64 -- or None."""
    from ._hip import NARROW_KINDS
    if isinstance(arr, np.ndarray) and arr.ndim == 2 and arr.flags.c_contiguous:
        return NARROW_KINDS.get(arr.dtype)
    return None


def load_gauges(gauges_file, observed_file, nmonths, missing=None):
    """Stream gauges of [Calibrate]: ``gauges_file`` rows gauge_id,cell_id[,weight] (cell_id 1-based; default weight 1),
    ``observed_file`` rows [gauge_id, *, *, value], ``nmonths`` rows per gauge in month order, NaN (or ``missing``) =
    no observation.  Returns calibrate.gauge_tables.Gauges (cells 0-based, obs [ngauge, nmonths])."""
    from .calibrate.gauge_tables import Gauges
    tab = np.atleast_2d(np.asarray(load_file(gauges_file, 0), dtype=float))
    if tab.shape[1] < 2:
        raise ValidationException('gauges: every row needs gauge_id,cell_id[,weight]')
    ids = tab[:, 0].astype(np.int64)
    weights = tab[:, 2] if tab.shape[1] > 2 else np.ones(ids.size)
    if isinstance(observed_file, str) and observed_file.endswith(('.csv', '.txt')):
        # (genfromtxt: an empty field is a missing observation too, not the 0 load_file fills in)
        rec = np.genfromtxt(observed_file, delimiter=',' if observed_file.endswith('.csv') else ' ')
    else:
        rec = load_file(observed_file, 0)
    rec = np.atleast_2d(np.asarray(rec, dtype=float))
    if rec.shape[1] < 4:
        raise ValidationException('gauge_observed: every row needs four columns, gauge id first and the value last')
    obs = np.full((ids.size, nmonths), np.nan)
    for i, g in enumerate(ids):
        rows = rec[rec[:, 0] == g][:nmonths, 3]
        if 0 < rows.size < nmonths:
            raise ValidationException('gauge_observed: gauge {} has {} rows, the run has {} months'.format(
                int(g), rows.size, nmonths))
        obs[i, :rows.size] = rows
    if missing is not None:
        obs[obs == missing] = np.nan
    return Gauges(ids, tab[:, 1].astype(np.int64) - 1, weights, obs)


def _present(f):
    return isinstance(f, np.ndarray) or (isinstance(f, str) and os.path.isfile(f))


def vectorize(data, ngridrow, ngridcol, map_index, skip=68):
    """2-D DRT map (rows north to south) -> per-cell vector (data_load.py:415-425)."""
    # row i of the map (south to north after the flip) lands on grid row i + skip; map_index addresses the grid in
    # column-major order, so cell k reads new[r, c] with r = map_index % ngridrow, c = map_index // ngridrow: one
    # index gather per cell instead of assembling (and re-ordering) the whole 360 x 720 grid
    data = np.asarray(data, dtype=float)
    map_index = np.asarray(map_index)
    r, c = map_index % ngridrow, map_index // ngridrow
    src = data.shape[0] - 1 - (r - skip)
    inside = (r >= skip) & (r < skip + data.shape[0])
    out = np.full(map_index.shape, -9999.0)
    out[inside] = data[src[inside], c[inside]]
    return out


class DataLoader:
    """Arrays the three plugins need, as attributes with the reference's names."""

    def __init__(self, s):
        self.s = s
        self.area = np.asarray(load_file(s.Area), dtype=float).reshape(-1) * 0.01
        self.coords = np.asarray(load_file(s.Coord), dtype=float)
        self.basin_ids = np.asarray(load_file(s.BasinIDs, 1)).reshape(-1).astype(int)
        self.latitude = np.copy(self.coords[:, 2])
        names = getattr(s, 'BasinNames', None)                   # one basin name per line (data_load.py:57, :366-368)
        if names and os.path.isfile(names):
            with open(names) as fh:
                self.basin_names = np.array(fh.read().splitlines())
        else:
            self.basin_names = np.array(['basin_{}'.format(k) for k in range(1, s.n_basins + 1)])
        # GCAM region and country maps with their names (data_load.py:59-69, :275-286): only read by the spatial
        # aggregation of the writer, so they are loaded when present and demanded only if that aggregation is on
        self.region_ids = self.region_names = self.country_ids = self.country_names = None
        rid, rnm = getattr(s, 'GCAMRegionIDs', None), getattr(s, 'GCAMRegionNames', None)
        if _present(rid) and _present(rnm):
            self.region_ids = np.asarray(load_file(rid, 1)).reshape(-1).astype(int)
            with open(rnm) as fh:
                fh.readline()
                self.region_names = np.array([ln.split(',')[0] for ln in fh.read().split('\n') if ln != ''])
        cid, cnm = getattr(s, 'CountryIDs', None), getattr(s, 'CountryNames', None)
        if _present(cid) and _present(cnm):
            self.country_ids = np.asarray(load_file(cid, 1)).reshape(-1).astype(int)
            with open(cnm) as fh:
                self.country_names = np.array([ln.split(',')[1] for ln in fh.read().splitlines()])
        if getattr(s, 'AggregateRunoffGCAMRegion', 0) and self.region_ids is None:
            raise ValidationException('AggregateRunoffGCAMRegion = 1 needs region32_grids.csv and Rgn32Names.csv in '
                                      'the reference directory')
        if getattr(s, 'AggregateRunoffCountry', 0) and self.country_ids is None:
            raise ValidationException('AggregateRunoffCountry = 1 needs country.csv and country-names.csv in the '
                                      'reference directory')
        # the diagnostics and the time-series plots read the maps of the scales they are asked for
        # (diagnostics.py:84-94, time_series.py:52-68)
        need_region = need_country = False
        if getattr(s, 'PerformDiagnostics', 0):
            need_country |= s.DiagnosticScale in (0, 2)
            need_region |= s.DiagnosticScale in (0, 3)
        if getattr(s, 'CreateTimeSeriesPlot', 0):
            need_country |= s.TimeSeriesScale not in (1, 3)
            need_region |= s.TimeSeriesScale not in (1, 2)
        if need_region and self.region_ids is None:
            raise ValidationException('the diagnostics / time-series scale asked for needs region32_grids.csv and '
                                      'Rgn32Names.csv in the reference directory')
        if need_country and self.country_ids is None:
            raise ValidationException('the diagnostics / time-series scale asked for needs country.csv and '
                                      'country-names.csv in the reference directory')
        # comparison runoff of the diagnostics (data_load.py:216-220)
        self.vic = self.unh = self.wbmd = self.wbmc = None
        if getattr(s, 'PerformDiagnostics', 0):
            self.vic = np.asarray(load_file(s.VICDataFile, 0, 'q'), dtype=float)
            self.unh = np.asarray(load_file(s.UNHDataFile, 0, 'q'), dtype=float)
            self.wbmd = np.asarray(load_file(s.WBMDataFile, 0, 'q'), dtype=float)
            self.wbmc = np.asarray(load_file(s.WBMCDataFile, 0, 'q'), dtype=float)

        if s.pet_module == 'pm':
            et = np.asarray(load_file(s.pm_params), dtype=float)
            (self.cL, self.beta, self.rslimit, self.ae, self.be, self.Tminopen, self.Tminclose, self.VPDclose,
             self.VPDopen, self.RBLmin, self.RBLmax, self.rc, self.emiss) = (et[:, k] for k in range(13))
            self.alpha = np.asarray(load_file(s.pm_alpha), dtype=float)
            self.lai = np.asarray(load_file(s.pm_lai), dtype=float)
            self.laimax = np.asarray(load_file(s.pm_laimax), dtype=float)
            self.laimin = np.asarray(load_file(s.pm_laimin), dtype=float)
            self.tair_load = self.load_to_array(s.pm_tas, 'pm_tas', nan_to_num=True)
            self.TMIN_load = self.load_to_array(s.pm_tmin, 'pm_tmin', nan_to_num=True)
            self.rhs_load = self.load_to_array(s.pm_rhs, 'pm_rhs', nan_to_num=True)
            self.wind_load = self.load_to_array(s.pm_wind, 'pm_wind', nan_to_num=True)
            self.rsds_load = self.load_to_array(s.pm_rsds, 'pm_rsds', nan_to_num=True)
            self.rlds_load = self.load_to_array(s.pm_rlds, 'pm_rlds', nan_to_num=True)
            self._tairprev = None        # tairprev_load: built on first use (the device pipeline derives it in HBM)
            self.lct_load = np.nan_to_num(load_file(s.pm_lct))
            self.elev = np.nan_to_num(load_file(s.pm_elev))
        elif s.pet_module == 'hargreaves':
            # temperature and daily temperature range (data_load.py:74-84): memory maps, untouched on the host -- the
            # negative-DTR clamp and nan_to_num of both (components.py:144-187) run in the Hargreaves kernel
            self.temp = self.load_to_array(s.TemperatureFile, 'TemperatureFile', key=getattr(s, 'TempVarName', None))
            self.dtr = self.load_to_array(s.DailyTemperatureRangeFile, 'DailyTemperatureRangeFile',
                                          key=getattr(s, 'DTRVarName', None))
        elif s.pet_module == 'hs':
            self.hs_tas = self.load_to_array(s.hs_tas, 'hs_tas')
            self.hs_tmin = self.load_to_array(s.hs_tmin, 'hs_tmin')
            self.hs_tmax = self.load_to_array(s.hs_tmax, 'hs_tmax')
        elif s.pet_module == 'thornthwaite':
            self.tair = self.load_to_array(s.trn_tas, 'trn_tas', nan_to_num=True)
        elif s.pet_module == 'none':
            self.pet_out = self.load_to_array(s.pet_file, 'pet_file')
        self.lat_radians = np.radians(self.latitude)          # data_load.py:71-72

        if s.runoff_module == 'abcd':
            self.precip = self.load_to_array(s.PrecipitationFile, 'PrecipitationFile', key=getattr(s, 'PrecipVarName', None))
            self.tmin = None if s.TempMinFile is None else self.load_to_array(
                s.TempMinFile, 'TempMinFile', nan_to_num=True, key=getattr(s, 'TempMinVarName', None))

        elif s.runoff_module == 'gwam':
            self.precip = self.load_to_array(s.PrecipitationFile, 'PrecipitationFile', key=getattr(s, 'PrecipVarName', None))
            self.soil_moisture, self.sm_prev = self.load_soil_moisture()

        if s.routing_module == 'mrtm':
            self.flow_dist = self.load_routing_data(s.flow_distance, rep_val=1000)
            self.flow_dir = self.load_routing_data(s.flow_direction)
            self.str_velocity = self.load_routing_data(s.strm_veloc, rep_val=0)
            # [[mrtm]] velocity_scale: every cell's velocity times its basin's scale, here, so that the routing plans, the
            # calibration tables and the hydropower post-processors all see the scaled array; velocity_scale [n_basins] is
            # what was loaded (ones without a file), which a calibration of the velocity multiplies into what it writes
            self.velocity_scale = np.ones(int(s.n_basins))
            if getattr(s, 'velocity_scale_file', None) is not None:
                from .calibrate.velocity_scale import apply_velocity_scale, read_velocity_scale
                self.velocity_scale = read_velocity_scale(s.velocity_scale_file, int(s.n_basins), '[[mrtm]] velocity_scale')
                self.str_velocity = apply_velocity_scale(self.str_velocity, self.basin_ids, self.velocity_scale)
            self.instream_flow = np.zeros((s.ncell,), dtype=float)
            self.chs_prev = self.load_chs_data()

        if s.calibrate:
            self.cal_obs = None if s.cal_observed is None else np.asarray(load_file(s.cal_observed, 0))[:, [0, 3]]
            self.gauges = None
            if getattr(s, 'cal_gauges', None) is not None:
                self.gauges = load_gauges(s.cal_gauges, s.cal_gauge_observed, s.nmonths,
                                          getattr(s, 'cal_gauge_missing', None))

    @property
    def tairprev_load(self):
        """Previous-row air temperature (data_load.py:127-128: zeros_like, then rows 1.. = rows ..-1 of tair_load)."""
        if self._tairprev is None:
            self._tairprev = np.zeros(self.tair_load.shape)
            self._tairprev[1:, :] = np.nan_to_num(np.asarray(self.tair_load[:-1, :], dtype=float))
        return self._tairprev

    @tairprev_load.setter
    def tairprev_load(self, v):
        self._tairprev = v

    def load_chs_data(self):
        """Initial channel storage (data_load.py:427-438): zeros in historic mode; in future mode the last column of the
        historical run's channel storage file."""
        s = self.s
        f = getattr(s, 'ChStorageFile', None)
        if str(getattr(s, 'HistFlag', 'True')) == 'True' or f is None:
            return np.zeros((s.ncell,), dtype=float)
        arr = np.asarray(load_file(f, 0, getattr(s, 'ChStorageVarName', None)), dtype=float)
        if arr.ndim == 1:
            arr = arr[:, None]
        if arr.shape[0] != s.ncell:
            raise ValidationException('ChStorageFile has {} cells, expected {}'.format(arr.shape[0], s.ncell))
        return np.ascontiguousarray(arr[:, -1])

    def load_soil_moisture(self):
        """GWAM's maximum soil moisture and initial soil moisture (data_load.py:149-182, :226-260): the max_soil_moisture
        table (one header row), overwritten at the water bodies of the two 1-based (cell, value) tables, lakes_msm and
        addit_water_msm (values truncated to integers, 999 marks a water body); initial soil moisture half of it in
        historic mode, the last column of SavFile in future mode."""
        s = self.s
        sm = np.asarray(load_file(s.max_soil_moisture, 1), dtype=float).reshape(-1).copy()
        if sm.shape[0] != s.ncell:
            raise ValidationException('max_soil_moisture has {} cells, expected {}'.format(sm.shape[0], s.ncell))
        for f in (s.lakes_msm, s.addit_water_msm):
            tab = np.asarray(load_file(f), dtype=float).reshape(-1, 2).astype(int)
            cells = tab[:, 0] - 1
            if cells.size and (cells.min() < 0 or cells.max() >= s.ncell):
                raise ValidationException('{}: cell ids outside 1..{}'.format(f, s.ncell))
            sm[cells] = tab[:, 1]
        if str(getattr(s, 'HistFlag', 'True')) == 'True':
            return sm, 0.5 * sm
        sav = np.asarray(load_file(s.SavFile, 0, getattr(s, 'SavVarName', None)), dtype=float)
        if sav.ndim == 1:
            sav = sav[:, None]
        if sav.shape[0] != s.ncell:
            raise ValidationException('SavFile has {} cells, expected {}'.format(sav.shape[0], s.ncell))
        return sm, np.ascontiguousarray(sav[:, -1])

    def load_to_array(self, f, var_name, nan_to_num=False, key=None):
        # the big forcing files stay on disk as read-only memory maps (mmap_inputs = False restores host arrays)
        lazy = getattr(self.s, 'device_transforms', True) and getattr(self.s, 'mmap_inputs', True)
        arr = load_file(f, key=key, mmap=lazy)
        # single precision and NetCDF's big-endian values stay AS STORED when nothing but DevicePipeline.set_forcing will
        # read them: their bytes cross PCIe and xh_widen makes the doubles in HBM (exact, so no result changes).  Every run
        # that hands the forcing to host code gets float64 here as before -- host code would compute in single precision
        if not (self.keeps_stored() and stored_kind(arr) is not None):
            arr = np.asanyarray(arr, dtype=float)      # a float64 memory map stays one
        # np.nan_to_num of the big forcing arrays (data_load.py:120-125, :194-195) is applied on the device right after
        # the upload (xh_nan_to_num) unless device_transforms is switched off: a host pass over 2.6 GB costs seconds
        if nan_to_num and not getattr(self.s, 'device_transforms', True):
            arr = np.nan_to_num(arr)
        if arr.shape[0] != self.s.ncell or arr.shape[1] != self.s.nmonths:
            raise ValidationException('Error: Inconsistent {0} data grid size. Expecting size: {1}. Received size: {2}'
                                      .format(var_name, (self.s.ncell, self.s.nmonths), arr.shape))
        return arr

    def keeps_stored(self):
        """Whether this run consumes its forcing only through DevicePipeline.set_forcing: a device-resident configuration
        (components.runs_device_resident, the predicate of the ensemble) without calibration, with the device transforms
        and the memory-mapped inputs on.  Stage-by-stage runs and the calibration read the arrays on the host."""
        s = self.s
        if not (getattr(s, 'device_transforms', True) and getattr(s, 'mmap_inputs', True)) or getattr(s, 'calibrate', 0):
            return False
        from .components import runs_device_resident
        from .configurations import ConfigRunner
        return runs_device_resident(s, getattr(s, 'pet_module', None) in ConfigRunner.PET_COMPONENTS,
                                    getattr(s, 'runoff_module', None) in ConfigRunner.RUNOFF_COMPONENTS)

    def load_routing_data(self, fn, rep_val=None):
        """Per-cell vector from a 1-D array or a 2-D DRT map (data_load.py:392-413)."""
        fd = np.asarray(load_file(fn), dtype=float)
        if fd.ndim == 2 and fd.shape[1] == self.s.ngridcol:
            r = self.coords[:, 4].astype(int) - 1
            c = self.coords[:, 3].astype(int) - 1
            map_index = np.ravel_multi_index((r, c), (self.s.ngridrow, self.s.ngridcol), order='F')
            # the DRT maps cover 280 of the 360 rows and sit 68 rows up from the bottom (data_load.py:392, skip=68)
            skip = 68 if (fd.shape[0] == 280 and self.s.ngridrow == 360) else self.s.ngridrow - fd.shape[0]
            v = vectorize(fd, self.s.ngridrow, self.s.ngridcol, map_index, skip=skip)
        else:
            v = fd.reshape(-1).copy()
        if v.shape[0] != self.s.ncell:
            raise ValidationException('routing input {} has {} cells, expected {}'.format(fn, v.shape[0], self.s.ncell))
        if rep_val is not None:
            v[v < rep_val] = rep_val
        return v
